// renderer.cpp -- the C-ABI of include/arctic_hip.h: resource ownership + frame graph on one HIP stream.
// The units of the C-ABI: renderer.cpp -- create, destroy and resize, streams, resources, the passes and frames, options, the debug read-backs;
// ray_calls.cpp -- queries, refit and re-split, sun visibility, ambient occlusion, hit attributes and shading, reflections, the composition, the
// motion vectors; exchange_calls.cpp -- the multi-GPU exchange (include/arctic_dist.h); taa_calls.cpp, motion_blur_calls.cpp, dof_calls.cpp,
// bloom_calls.cpp, exposure_calls.cpp, fog_calls.cpp, taa_upscale_calls.cpp -- one post stage each; post_source.cpp -- what those stages share.
// The handle they share: renderer_state.h.
//
// Plays the role of Arctic::Renderer::Renderer (reference src/renderer/renderer.{hpp,cpp}) for
// the hot path only: create_material/create_mesh/update_lights upload resources
// (renderer.cpp:417-603), render_frame runs shadow-map raster -> visibility/G-buffer prepass ->
// shading+tonemap (renderer.cpp:285-357 minus skybox, ImGui and present).  Everything D3D12
// (RHI, descriptor heaps, barriers, swapchain) is replaced by plain device allocations and
// stream order.  No CPU fallback: every entry point needs a HIP device.
#include <algorithm>
#include <cstdio>

#include <cstdlib>
#include <cstring>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/arctic_hip.h"
#include "../../include/arctic_dist.h"
#include "common.h"
#include "device_resources.h"
#include "renderer_state.h"

using namespace arctic;

namespace arctic {
Markers g_markers;
}  // namespace arctic

namespace {

// Object-space boxes for geometry.hip's box_outside, made once per mesh on the host (arctic_cluster_bounds is this function).
// tbounds[c] = {min xyz, max xyz} of the positions the valid triangles [c * SETUP_THREADS, (c + 1) * SETUP_THREADS) use -- one workgroup of
// k_setup.  vbounds[b] = the union of tbounds[t / SETUP_THREADS] over every valid triangle t that uses one of the vertices [256 b, 256 b + 256)
// -- one workgroup of k_vertex --, made in a second pass over the finished tbounds: a vertex block's box CONTAINS the box of every cluster
// that reads one of its vertices, which is what lets k_vertex skip it (box_outside's comment has the argument).  The union of the boxes of
// those TRIANGLES alone is smaller than their clusters' boxes and is not enough.
// Triangles with an index out of range draw nothing (load_indices) and bound nothing.  A cluster with a position that is not finite, or with no
// valid triangle, gets an infinite box (never culled); a block that touches such a cluster, or that no valid triangle uses, gets one too.
void cluster_bounds(const ArcticVertex *v, uint32_t n_vertices, const uint32_t *ind, uint32_t n_indices, std::vector<float> &tb, std::vector<float> &vb) {
    const uint32_t n_tri = n_indices / 3, n_tb = (n_tri + SETUP_THREADS - 1) / SETUP_THREADS, n_vb = (n_vertices + 255) / 256;
    const float inf = std::numeric_limits<float>::infinity();
    tb.assign((size_t)n_tb * 6, 0.0f); vb.assign((size_t)n_vb * 6, 0.0f);
    for (uint32_t b = 0; b < n_tb; ++b) for (int k = 0; k < 3; ++k) { tb[6 * b + k] = inf; tb[6 * b + 3 + k] = -inf; }
    for (uint32_t b = 0; b < n_vb; ++b) for (int k = 0; k < 3; ++k) { vb[6 * b + k] = inf; vb[6 * b + 3 + k] = -inf; }
    const auto valid = [&](uint32_t t) { return ind[3 * t] < n_vertices && ind[3 * t + 1] < n_vertices && ind[3 * t + 2] < n_vertices; };
    const auto open_unless_bounded = [&](std::vector<float> &box, uint32_t b, bool bad) {   // (an untouched box still has min = inf > max = -inf)
        if (bad || !(box[6 * b] <= box[6 * b + 3])) for (int k = 0; k < 3; ++k) { box[6 * b + k] = -inf; box[6 * b + 3 + k] = inf; }
    };
    std::vector<char> bad_t(n_tb, 0);
    for (uint32_t t = 0; t < n_tri; ++t) {
        if (!valid(t)) continue;
        const uint32_t c = t / SETUP_THREADS;
        for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) {
            const float p = v[ind[3 * t + j]].position[k];
            if (!std::isfinite(p)) bad_t[c] = 1;
            tb[6 * c + k] = std::min(tb[6 * c + k], p); tb[6 * c + 3 + k] = std::max(tb[6 * c + 3 + k], p);
        }
    }
    for (uint32_t c = 0; c < n_tb; ++c) open_unless_bounded(tb, c, bad_t[c] != 0);
    // second pass: every box of tb is now final, finite or {-inf, inf}; min / max carry an infinite box into the block's
    for (uint32_t t = 0; t < n_tri; ++t) {
        if (!valid(t)) continue;
        const uint32_t c = t / SETUP_THREADS;
        for (int j = 0; j < 3; ++j) {
            const uint32_t b = ind[3 * t + j] / 256;
            for (int k = 0; k < 3; ++k) { vb[6 * b + k] = std::min(vb[6 * b + k], tb[6 * c + k]); vb[6 * b + 3 + k] = std::max(vb[6 * b + 3 + k], tb[6 * c + 3 + k]); }
        }
    }
    for (uint32_t b = 0; b < n_vb; ++b) open_unless_bounded(vb, b, false);
}

}  // namespace

namespace arctic {   // (renderer_state.h: other units call these)

// bytes of a shadow-map buffer: S rows, or -- with a communicator -- world * ceil(S / world) rows, the room the in-place all-gather
// of a sharded map writes (ARCTIC_OPT_SHADOW_SHARDED); + 8: the map is cleared in 8-byte words.  ONE definition for every place
// that allocates a map (arctic_create, the second map of frames in flight, arctic_comm_init).
size_t shadow_alloc_bytes(const ArcticRenderer *r) {
    const uint32_t S = r->shadow_size, w = (uint32_t)std::max(1, r->comm_world);
    const uint32_t rows = std::max(S, w * ((S + w - 1) / w));
    return (size_t)rows * S * 4 + 8;
}

int select_device(ArcticRenderer *r) {
    HIPCHECK(r, hipSetDevice(r->device));
    return ARCTIC_OK;
}

}  // namespace arctic

namespace {

int alloc_targets(ArcticRenderer *r) {
    r->shadow_key.clear();   // buffers may move: render_frame redraws the shadow map
    shard_tile_rows(r->height, r->row_begin, r->row_end, r->band_rows, r->shard_index, r->shard_count, r->tile_y0, r->tiles_y);
    r->row0_in_tile = r->row_begin - r->tile_y0 * TILE;
    r->tiles_x = (r->width + TILE - 1) / TILE;
    if (r->band_rows) {   // interleaved shard: count the pixel rows this shard owns
        const int bt = (int)(r->band_rows / TILE), all = (int)((r->height + TILE - 1) / TILE);
        uint32_t own_r = 0;
        for (int ty = 0; ty < all; ++ty)
            if (row_owned(ty, bt, (int)r->shard_count, (int)r->shard_index)) own_r += std::min<uint32_t>(TILE, r->height - (uint32_t)ty * TILE);
        r->owned_rows = own_r;
    }
    size_t px = r->n_tiles() * TILE_PIXELS, out_px = (size_t)r->rows() * r->width;
    for (DevBuf &v : r->d_vis_set) HIPCHECK(r, v.ensure(px * 8));
    // the library's choice of frames in flight: 2, and 3 for targets below 3 Mpx, whose prepass -- a chain of launches -- is longer than
    // their shading (tools/experiments/in_flight.py, 2 / 3 in flight: 1080p config 2 0.077 / 0.065 ms, config 3 at 1080p 0.094 / 0.088,
    // config 1 0.030 / 0.026; 4K 0.278 / 0.284)
    if (r->frames_in_flight_opt == 0) { r->frames_in_flight = (uint64_t)r->rows() * r->width < 3000000ull ? 3 : 2; r->cur = 0; }
    for (StreamMark &m : r->vis_set_released) m.forget();   // (callers synchronise before they resize)
    HIPCHECK(r, r->d_p0.ensure(px * 16));
    HIPCHECK(r, r->d_p1.ensure(px * 16));
    HIPCHECK(r, r->d_p2.ensure(px * 16));
    HIPCHECK(r, r->d_p3.ensure(px * 16));
    HIPCHECK(r, r->d_p4.ensure(px * 12));
    if (r->texture_mips) HIPCHECK(r, r->d_lod.ensure(px * 4));
    r->lod_valid = false;
    HIPCHECK(r, r->d_rgba8.ensure(out_px * 4));
    HIPCHECK(r, r->d_counter.ensure(8 * N_SHADE_STATS));
    HIPCHECK(r, r->d_geo_counters.ensure(5 * N_GEO_COUNTERS * 4));   // N_GEO_COUNTERS words per table set; set 4: the cube faces (CUBE_COUNTER_SET)
    r->have_gbuffer = r->have_output = r->have_vis = r->have_order = false;
    r->hdr_valid = false;
    r->compose.pixels = 0;   // (arctic_read_composed: nothing composed at this size yet)
    r->ao_history.valid = false;   // (the occlusion's history is empty after a resize)
    r->motion.valid = false;       // (... and so is what the previous motion call saw)
    r->taa.valid = false;          // (... and the anti-aliasing's T; the camera jitter stays)
    r->motion_blur.valid = false;  // (... and what the latest motion blur left)
    r->dof.valid = false;          // (... and the latest depth of field)
    r->bloom.valid = false;        // (... and the latest bloom)
    r->exposure.valid = r->exposure.planes = false;   // (... and the exposure's adaptation and planes)
    r->fog.valid = false;          // (... and the latest fog)
    r->taa_upscale.valid = false;  // (... and the upscaler's U)
    r->gi.pixels = r->gi.composed = 0; r->gi.hist_valid = false;   // (... and the latest indirect light, its history and its composition)
    r->output_filtered = false;
    return ARCTIC_OK;
}

// Scene.objects -> ObjectRec[] + block tables in one asynchronous upload, skipped while the list stays byte-identical (a
// static scene under a moving camera: the frame constants travel as a kernel argument, so such frames copy nothing)
int upload_pass_tables(ArcticRenderer *r, PassTables &T, DevBuf &d_xverts, hipStream_t stream, const GeomParams &gp, const ArcticScene *sc, uint32_t &n_objs,
                       uint32_t &n_xverts, uint32_t &n_src_tris, uint32_t &n_vblocks, uint32_t &n_tblocks) {
    std::vector<ObjectRec> objs;
    std::vector<uint32_t> vb_obj, vb_first, tb_obj, tb_first;
    std::vector<float> vb_box, tb_box;
    uint64_t xv = 0, tri = 0;
    for (uint64_t i = 0; i < sc->n_objects; ++i) {
        const ArcticObject &o = sc->objects[i];
        if (o.mesh_idx >= r->meshes.size()) continue;   // the reference would index out of bounds; skipped here
        const Mesh &m = r->meshes[o.mesh_idx];
        ObjectRec rec;
        std::memcpy(rec.trs, o.trs, sizeof rec.trs);
        rec.vertices = m.vertices_in_use();
        rec.indices = m.d_indices.as<uint32_t>();
        rec.n_vertices = m.n_vertices;
        rec.n_triangles = m.n_indices / 3;
        rec.first_xvert = (uint32_t)xv;
        rec.first_triangle = (uint32_t)tri;
        rec.material = (uint32_t)m.material;
        rec.pad = 0;
        uint32_t oi = (uint32_t)objs.size();
        for (uint32_t b = 0; b < rec.n_vertices; b += 256) { vb_obj.push_back(oi); vb_first.push_back(b); }
        for (uint32_t b = 0; b < rec.n_triangles; b += SETUP_THREADS) { tb_obj.push_back(oi); tb_first.push_back(b); }
        if (m.deformed()) {   // the boxes bound the mesh's own shape: a posed or morphed mesh gets cluster_bounds' "cannot bound" boxes, which are never skipped
            const float inf = std::numeric_limits<float>::infinity(), open_box[6] = {-inf, -inf, -inf, inf, inf, inf};
            for (size_t b = 0; b < m.vbounds.size() / 6; ++b) vb_box.insert(vb_box.end(), open_box, open_box + 6);
            for (size_t b = 0; b < m.tbounds.size() / 6; ++b) tb_box.insert(tb_box.end(), open_box, open_box + 6);
        } else {
            vb_box.insert(vb_box.end(), m.vbounds.begin(), m.vbounds.end());
            tb_box.insert(tb_box.end(), m.tbounds.begin(), m.tbounds.end());
        }
        xv += rec.n_vertices;
        tri += rec.n_triangles;
        objs.push_back(rec);
    }
    if (xv > 0xFFFFFFF0ull || tri > 0xFFFFFFF0ull) return r->fail(ARCTIC_E_CAPACITY, "scene too large: %llu vertices, %llu triangles", (unsigned long long)xv, (unsigned long long)tri);
    n_objs = (uint32_t)objs.size(); n_xverts = (uint32_t)xv; n_src_tris = (uint32_t)tri;
    n_vblocks = (uint32_t)vb_obj.size(); n_tblocks = (uint32_t)tb_obj.size();
    // arena layout (16-byte aligned sections)
    auto align16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_objs = 0, o_vo = align16(o_objs + objs.size() * sizeof(ObjectRec)),
                 o_vf = align16(o_vo + vb_obj.size() * 4), o_to = align16(o_vf + vb_first.size() * 4),
                 o_tf = align16(o_to + tb_obj.size() * 4), o_vb = align16(o_tf + tb_first.size() * 4), o_tb = align16(o_vb + vb_box.size() * 4),
                 total = align16(o_tb + tb_box.size() * 4) + 16;
    if (vb_box.size() != vb_obj.size() * 6 || tb_box.size() != tb_obj.size() * 6) return r->fail(ARCTIC_E_INVALID, "internal: cluster bounds out of step with the block tables");
    T.gp = gp;
    std::vector<char> stage(total, 0);
    char *h = stage.data();
    if (!objs.empty()) std::memcpy(h + o_objs, objs.data(), objs.size() * sizeof(ObjectRec));
    if (!vb_obj.empty()) { std::memcpy(h + o_vo, vb_obj.data(), vb_obj.size() * 4); std::memcpy(h + o_vf, vb_first.data(), vb_first.size() * 4); }
    if (!tb_obj.empty()) { std::memcpy(h + o_to, tb_obj.data(), tb_obj.size() * 4); std::memcpy(h + o_tf, tb_first.data(), tb_first.size() * 4); }
    if (!vb_box.empty()) std::memcpy(h + o_vb, vb_box.data(), vb_box.size() * 4);
    if (!tb_box.empty()) std::memcpy(h + o_tb, tb_box.data(), tb_box.size() * 4);
    if (!(T.d.p && stage == T.last)) {
        char *pinned = nullptr;
        HIPCHECK(r, T.staging.stage(T.staging.slot[0].h.cap < total ? total * 2 : total, &pinned));   // (a slot that has to grow gets twice the table)
        T.last.clear();
        HIPCHECK(r, T.d.ensure(total));
        std::memcpy(pinned, h, total);
        HIPCHECK(r, T.staging.send(T.d.p, total, stream));
        T.last.swap(stage);
    }
    const char *d = T.d.as<char>();
    T.objs = reinterpret_cast<const ObjectRec *>(d + o_objs);
    T.vblock_obj = reinterpret_cast<const uint32_t *>(d + o_vo); T.vblock_first = reinterpret_cast<const uint32_t *>(d + o_vf);
    T.tblock_obj = reinterpret_cast<const uint32_t *>(d + o_to); T.tblock_first = reinterpret_cast<const uint32_t *>(d + o_tf);
    T.vblock_bounds = reinterpret_cast<const float *>(d + o_vb); T.tblock_bounds = reinterpret_cast<const float *>(d + o_tb);
    if (n_objs) {
        HIPCHECK(r, d_xverts.ensure((size_t)n_xverts * sizeof(XVert)));
    }
    return ARCTIC_OK;
}

// A depth-only target other than the sun's map: one face of a shadow-casting point light (pass_point_shadows).  It is drawn like the
// sun's map -- front faces culled, depth LESS, cleared to 1.0, small triangles by k_setup -- with the shadow pass's scratch (geo[1],
// tables[1]), but counts into slots of its own, so that arctic_stats and arctic_read_cull_counts keep describing the sun's pass; and
// it never takes block owners, a sharded map or k_vertex's block culling (left off while a vertex block's box was made of triangle boxes, ADVICE.md, and not measured with it since)
constexpr uint32_t CUBE_COUNTER_SET = 4;   // its set of N_GEO_COUNTERS device counters
constexpr uint32_t CUBE_COUNT_WORDS = 8;   // pinned words per face: [0] records, [1] work items, [2] overflow flag, [4] items of the atomic rasteriser (k_raster)
struct DepthTarget {
    uint32_t *map;                  // size x size floats
    uint32_t size;
    const float *clip_from_world;   // 16 floats, glm memory order
    uint32_t *h_counts, *dh_counts; // CUBE_COUNT_WORDS pinned words: host and device address
};

// vertex -> clip/setup -> raster, shared by the forward prepass, the shadow pass and (cube != null) the faces of the point lights
int run_geometry(ArcticRenderer *r, const ArcticScene *sc, bool shadow_pass, hipStream_t stream, const DepthTarget *cube = nullptr) {
    const int set = shadow_pass ? 1 : r->fwd();
    const uint32_t cset = cube ? CUBE_COUNTER_SET : (uint32_t)set;   // counter set
    ArcticRenderer::GeoSet &G = r->geo[set];
    const uint32_t S = cube ? cube->size : r->shadow_size;   // a depth target's side
    uint32_t *depth_map = cube ? cube->map : r->d_shadow().as<uint32_t>();
    // the pass's target is cleared by the vertex kernel's launch (or by a fill when there is nothing to draw)
    unsigned long long *clear = shadow_pass ? reinterpret_cast<unsigned long long *>(depth_map) : r->d_vis().as<unsigned long long>();
    const unsigned long long clear_value = shadow_pass ? 0x3F8000003F800000ull : ~0ull;   // depth 1.0 (shadow_map_pass.cpp:124-131) / no triangle
    const size_t clear_count = shadow_pass ? ((size_t)S * S + 1) / 2 : r->n_tiles() * TILE_PIXELS;
    GeomParams gp;
    std::memset(&gp, 0, sizeof gp);
    sun_proj_view(sc->sun.position, sc->sun.rotation, gp.light_from_world);
    if (shadow_pass) {
        std::memcpy(gp.clip_from_world, cube ? cube->clip_from_world : gp.light_from_world, sizeof gp.clip_from_world);
        gp.vp_w = gp.vp_h = (float)S;
        gp.sc_x0 = gp.sc_y0 = 0; gp.sc_x1 = gp.sc_y1 = (int32_t)S;
        if (!cube && r->shadow_sharded && r->comm && r->comm_world > 1) {   // this rank's slice of the light-space rows; the all-gather follows the raster
            const uint32_t per = (r->shadow_size + (uint32_t)r->comm_world - 1) / (uint32_t)r->comm_world;
            gp.sc_y0 = (int32_t)std::min(r->shadow_size, per * (uint32_t)r->comm_rank);
            gp.sc_y1 = (int32_t)std::min(r->shadow_size, per * ((uint32_t)r->comm_rank + 1));
        }
        gp.cull_front = 1;                                       // shadow_map_pass.cpp:96-97
        gp.tiles_x = (int32_t)((S + 7) / 8); gp.tile_y0 = 0; gp.pitch = (int32_t)S;
    } else {
        const ArcticCamera &c = sc->camera;
        camera_proj_view(c.eye, c.rotation, c.aspect, c.fov_y, c.z_near_far[0], c.z_near_far[1], gp.clip_from_world);
        // arctic_set_camera_jitter: the matrix that is DRAWN, from here on (the cluster culling below tests against it); with (0, 0) it is not touched
        if (r->taa.jitter[0] != 0.0f || r->taa.jitter[1] != 0.0f) (void)arctic_jitter_proj_view(gp.clip_from_world, r->width, r->height, r->taa.jitter[0], r->taa.jitter[1]);
        gp.vp_w = (float)r->width; gp.vp_h = (float)r->height;
        gp.sc_x0 = 0; gp.sc_x1 = (int32_t)r->width; gp.sc_y0 = (int32_t)r->row_begin; gp.sc_y1 = (int32_t)r->row_end;
        gp.cull_front = 0;                                       // forward_pass.cpp:143-144
        gp.tiles_x = (int32_t)r->tiles_x; gp.tile_y0 = (int32_t)r->tile_y0; gp.pitch = 0;
        gp.band_tiles = (int32_t)(r->band_rows / TILE); gp.shard_index = (int32_t)r->shard_index; gp.shard_count = (int32_t)r->shard_count;
    }
    gp.raster_flags = ((r->debug & 32) ? 1 : 0) | ((r->debug & 1024) ? 2 : 0);
    gp.tiles_y = shadow_pass ? (int32_t)((S + 7) / 8) : (int32_t)r->tiles_y;
    // block ownership (ARCTIC_OPT_RASTER_OWNER; default -1 = the choice below): the blocks are written once by their owners, so nothing is cleared
    // the library's choice: the forward pass of a handle that owns 4 Mpx or more -- three launches instead of one cost ~12 us of fixed
    // time, what the atomics cost grows with the pixels.  Whole frames with / without owners: 4K 0.283 / 0.304 ms, one rank of R = 2 at 4K
    // (4.1 Mpx) 0.178 / 0.184, of R = 4 0.136 / 0.130, of R = 8 0.106 / 0.102; config 3 at 1080p 0.113 / 0.114, config 2 (1080p, dense
    // meshes: 14 % of the items beyond their bins) 0.106 / 0.093, config 1 (512^2) 0.064 / 0.038;
    // never the shadow pass (instruction bound, two thirds of its blocks empty: 0.124 -> 0.163 ms)
    const bool owned = cube ? false : r->raster_owner < 0 ? (!shadow_pass && (uint64_t)r->rows() * r->width >= 4000000ull) : (r->raster_owner & (shadow_pass ? 2 : 1)) != 0;
    // owners beside the small-triangle path: the map is cleared as without owners, k_setup draws the small triangles into it, the owners MERGE their bins into it
    const bool merge = owned && shadow_pass && r->small_triangles && !(r->debug & 32);
    BinTables B{};
    if (owned) {
        const uint32_t tw = shadow_pass ? r->shadow_size : r->width, th = shadow_pass ? r->shadow_size : r->height;
        B.blocks_x = (tw + 15) / 16;
        B.n_blocks = B.blocks_x * ((th + 15) / 16);
        if (shadow_pass) { B.grid_x = B.blocks_x; B.by0 = 0; B.grid_y = (th + 15) / 16; B.local_rows = 0; }
        else owner_grid(tw, th, r->tile_y0, r->tiles_y, (uint32_t)gp.band_tiles, B.grid_x, B.grid_y, B.by0, B.local_rows);
        HIPCHECK(r, G.d_bin_count.ensure((size_t)B.n_blocks * 4));
        HIPCHECK(r, G.d_bin_slots.ensure((size_t)B.n_blocks * BIN_SLOTS * 4));
        B.count = G.d_bin_count.as<uint32_t>(); B.slots = G.d_bin_slots.as<uint32_t>();
        B.count_all = (r->debug & 512) ? 1u : 0u;
        G.bins_x = B.blocks_x; G.bins_y = B.n_blocks / B.blocks_x;
    } else if (!cube) G.bins_x = G.bins_y = 0;
    PassTables &T = r->tables[set];
    uint32_t n_objs, n_xverts, n_src, n_vblocks, n_tblocks;
    int rc = upload_pass_tables(r, T, G.d_xverts, stream, gp, sc, n_objs, n_xverts, n_src, n_vblocks, n_tblocks);
    if (rc != ARCTIC_OK) return rc;
    const GeomParams &d_gp = T.gp;
    uint32_t *hc = cube ? cube->h_counts : r->h_counts() + (shadow_pass ? 2 : 0);   // [0] records, [1] work items of the latest pass into this target
    if (n_objs == 0 || n_src == 0 || n_vblocks == 0) {
        hc[0] = hc[1] = 0;
        HIPCHECK(r, launch_fill_u64(clear, clear_value, clear_count, stream));
        return ARCTIC_OK;
    }
    const ObjectRec *objs = T.objs;
    const bool count_culls = (r->debug & 1024) != 0;
    if (!cube) { G.n_tblocks = n_tblocks; G.n_vblocks = n_vblocks; G.cull_counted = count_culls; }
    if (count_culls) HIPCHECK(r, hipMemsetAsync(r->d_geo_counters.as<uint32_t>() + N_GEO_COUNTERS * cset + 6, 0, 4, stream));   // (k_vertex counts into it from its first workgroup on)
    HIPCHECK(r, launch_vertex(objs, T.vblock_obj, T.vblock_first, n_vblocks, d_gp, G.d_xverts.as<XVert>(), shadow_pass ? 1 : 0,
                              r->d_geo_counters.as<uint32_t>() + N_GEO_COUNTERS * cset, clear, clear_value, (owned && !merge) ? 0 : clear_count, B.count, owned ? B.n_blocks : 0,
                              (r->cluster_cull & 2) && !cube ? T.vblock_bounds : nullptr, stream));
    // Record slots: a triangle clipped against 6 planes yields at most 7 triangles, so 7 * n_src slots can never overflow.
    // Records and work items are allocated on the device from two counters (k_setup): no count pass, no scan, and neither
    // count has to come back to the host -- the frame stays asynchronous.
    const uint64_t slots64 = 7ull * n_src;
    if (slots64 > 0x0FFFFFF0ull) return r->fail(ARCTIC_E_CAPACITY, "scene too large: %u triangles", n_src);
    // ... but 7 x 128 B per source triangle is a lot of memory for what only heavy clipping can produce: the table starts at
    // 2 records per source triangle and goes to the worst case only after a frame has overflowed it (flagged like the item table)
    const uint32_t n_slots = r->recs_worst_case ? (uint32_t)slots64 : (uint32_t)std::min<uint64_t>(slots64, 2ull * n_src + 4096);
    // work-item table: explicit (record, 16x16 block) pairs.  Its size follows the largest count seen so far (pinned
    // h_counts, refreshed asynchronously each pass) with 4x headroom; an overflow drops work, is flagged by the kernel and
    // reported by the next call that synchronises (arctic_flush / read-backs) -- and the table has grown by then.
    const uint64_t want = std::max<uint64_t>(r->item_cap_floor, 4ull * hc[1]);
    if (want > G.item_cap) {
        HIPCHECK(r, G.d_items.ensure((size_t)want * 8));
        G.item_cap = (uint32_t)std::min<uint64_t>(want, 0x7FFFFFF0ull);
    }
    if (owned) HIPCHECK(r, G.d_left.ensure((size_t)G.item_cap * 8));
    HIPCHECK(r, G.d_recs.ensure((size_t)n_slots * sizeof(SetupRec)));
    HIPCHECK(r, G.d_rrecs.ensure((size_t)n_slots * sizeof(RasterRec)));
    HIPCHECK(r, G.d_rec_of.ensure((size_t)n_src * 8 * 4));
    HIPCHECK(r, G.d_clip_list.ensure((size_t)n_src * 8));
    uint32_t *counters = r->d_geo_counters.as<uint32_t>() + N_GEO_COUNTERS * cset;   // zeroed by k_vertex
    HIPCHECK(r, launch_setup(objs, T.tblock_obj, T.tblock_first, n_tblocks, d_gp, G.d_xverts.as<XVert>(), G.d_recs.as<SetupRec>(),
                             G.d_rrecs.as<RasterRec>(), G.d_rec_of.as<uint32_t>(), G.d_items.as<uint2>(), G.item_cap, n_slots, counters,
                             G.d_clip_list.as<uint2>(), (r->cluster_cull & 1) ? T.tblock_bounds : nullptr,
                             // (block owners STORE their blocks -- that store is the clear --, so nothing may be drawn before them unless they merge)
                             shadow_pass && (!owned || merge) && r->small_triangles ? depth_map : nullptr, stream));
    // counts for arctic_stats() and the overflow flag: k_raster stores them into pinned, mapped memory (no copy launches between
    // the kernels); looked at only when the stream has been synchronised
    uint32_t *dh = cube ? cube->dh_counts : r->dh_counts() + (shadow_pass ? 2 : 0), *dh_overflow = cube ? cube->dh_counts + 2 : r->dh_counts() + 4 + (shadow_pass ? 1 : 0);
    uint32_t grid = r->raster_blocks[shadow_pass ? 1 : 0];
    const uint2 *draw = G.d_items.as<uint2>();
    if (owned) {
        HIPCHECK(r, launch_raster_owned(shadow_pass, G.d_rrecs.as<RasterRec>(), G.d_items.as<uint2>(), G.d_left.as<uint2>(), G.item_cap, counters, B, d_gp,
                                        shadow_pass ? nullptr : r->d_vis().as<unsigned long long>(), shadow_pass ? r->d_shadow().as<uint32_t>() : nullptr, merge, stream));
        // what the bins left goes through the atomic rasteriser: when the previous pass left next to nothing (pinned h_counts, a frame
        // late: it only sizes the grid) a launch of 64 workgroups, else the whole persistent grid -- the kernel shortens its chunks
        // so that every resident wave gets one (a grid cut to the item count measured slower: config 1, half of whose items are left)
        draw = G.d_left.as<uint2>();
        if (r->h_counts()[6 + (shadow_pass ? 1 : 0)] <= 64) grid = std::min<uint32_t>(grid, 64);
    }
    if (shadow_pass)
        HIPCHECK(r, launch_raster_depth(G.d_recs.as<SetupRec>(), G.d_rrecs.as<RasterRec>(), draw, G.item_cap, counters, grid, d_gp,
                                        depth_map, dh, dh_overflow, owned, stream));
    else
        HIPCHECK(r, launch_raster_vis(G.d_recs.as<SetupRec>(), G.d_rrecs.as<RasterRec>(), draw, G.item_cap, counters, grid, d_gp,
                                      r->d_vis().as<unsigned long long>(), dh, dh_overflow, owned, stream));
    return ARCTIC_OK;
}

// the min/max table of the shadow map (shade.hip: the test that replaces the 25 PCF taps for most pixels): rebuilt, two small
// launches, after the map was written
int build_shadow_bounds(ArcticRenderer *r, hipStream_t stream) {
    const uint32_t nb = shadow_bounds_pitch(r->shadow_size);
    if (!nb || r->bounds_valid()) return ARCTIC_OK;
    HIPCHECK(r, r->d_shadow_blocks().ensure((size_t)nb * nb * 8));
    HIPCHECK(r, r->d_shadow_bounds().ensure((size_t)nb * nb * 8));
    HIPCHECK(r, launch_shadow_bounds(r->d_shadow().as<float>(), r->shadow_size, r->d_shadow_blocks().as<float2>(), r->d_shadow_bounds().as<float2>(), stream));
    r->bounds_valid() = true;
    return ARCTIC_OK;
}

int pass_shadow_map(ArcticRenderer *r, const ArcticScene *sc, hipStream_t stream) {
    if (r->shadow_size == 0) return ARCTIC_OK;
    Range zone("Shadow Map Pass");
    r->bounds_valid() = false;
    HIPCHECK(r, r->shadow_scratch_free.wait(stream));   // the previous shadow pass ran on another stream: it owns the scratch until it ends
    int rc = run_geometry(r, sc, true, stream);
    HIPCHECK(r, r->shadow_scratch_free.record(stream));
    if (rc != ARCTIC_OK) return rc;
    r->shadow_written_set[r->scur] = true;
    if (r->shadow_sharded && r->comm && r->comm_world > 1) {
        // every rank has drawn ceil(S / world) rows of the map: one in-place all-gather (the send buffer is this rank's slice of the
        // receive buffer) completes it everywhere, on the pass's stream -- the shading pass needs it next
        const size_t per = (size_t)((r->shadow_size + (uint32_t)r->comm_world - 1) / (uint32_t)r->comm_world) * r->shadow_size;
        float *base = r->d_shadow().as<float>();
        if (r->d_shadow().cap < per * (size_t)r->comm_world * 4)   // (cannot happen through this API: every map is sized by shadow_alloc_bytes)
            return r->fail(ARCTIC_E_STATE, "sharded shadow map: the map buffer has no room for %d x %zu texels", r->comm_world, per);
        const int nrc = g_rccl.AllGather(base + per * (size_t)r->comm_rank, base, per, Rccl::Float32, r->comm, stream);
        if (nrc != 0) return r->fail(ARCTIC_E_DEVICE, "ncclAllGather(shadow map): %s", g_rccl.why(nrc));
    }
    return ARCTIC_OK;
}

// the faces of every shadow-casting point light (arctic_update_point_shadow_lights), 6 per light, each run_geometry's depth-only pass with
// the face's matrix (host_math.cpp point_shadow_proj_view).  On the pass's stream behind the shadow scratch's guard, like the sun's map:
// whole frames call it on the main stream, so the faces are redrawn after the previous frame's shading has read them
float *cube_faces(ArcticRenderer *r) { return reinterpret_cast<float *>(r->d_cubes.as<char>() + (size_t)r->n_cubes * sizeof(CubeDev)); }
int pass_point_shadows(ArcticRenderer *r, const ArcticScene *sc, hipStream_t stream) {
    if (!r->n_cubes) return ARCTIC_OK;
    Range zone("Point Shadow Pass");
    HIPCHECK(r, r->shadow_scratch_free.wait(stream));   // the previous shadow pass ran on another stream: it owns the scratch until it ends
    const size_t texels = (size_t)r->cube_size * r->cube_size;
    int rc = ARCTIC_OK;
    for (uint32_t i = 0; i < r->n_cubes && rc == ARCTIC_OK; ++i) {
        const ArcticPointShadowLight &l = r->cube_lights[i];
        for (int k = 0; k < 6 && rc == ARCTIC_OK; ++k) {
            float m[16];
            point_shadow_proj_view(l.position, k, l.z_near, l.z_far, m);
            const size_t j = (size_t)i * 6 + k;
            const DepthTarget t = {reinterpret_cast<uint32_t *>(cube_faces(r) + j * texels), r->cube_size, m,
                                   r->h_cube_counts() + CUBE_COUNT_WORDS * j, r->dh_cube_counts() + CUBE_COUNT_WORDS * j};
            rc = run_geometry(r, sc, true, stream, &t);
        }
    }
    HIPCHECK(r, r->shadow_scratch_free.record(stream));
    if (rc == ARCTIC_OK) r->cube_faces_filled = true;
    return rc;
}

// visibility only: vertex -> setup -> raster of the camera view
int pass_visibility(ArcticRenderer *r, const ArcticScene *sc, hipStream_t stream) {
    Range zone("Forward Pass: visibility");
    r->have_gbuffer = false; r->have_order = false;
    int rc = run_geometry(r, sc, false, stream);
    if (rc != ARCTIC_OK) return rc;
    r->have_vis = true;
    return ARCTIC_OK;
}

}  // namespace
namespace arctic {   // (renderer_state.h: other units call it)
// visibility -> the 76 B/pixel G-buffer.  Valid while the records of the forward pass are still in place.
int resolve_gbuffer(ArcticRenderer *r) {
    Range zone("Forward Pass: G-buffer");
    if (!r->have_vis)
        return r->fail(ARCTIC_E_STATE, "no G-buffer: no visibility plane to resolve it from (run arctic_pass_gbuffer)");
    // the cost classes need the shadow map's min/max table as the shading pass will read it (rebuilt here if the map was written since)
    TileHint hint = {nullptr, nullptr, 0, 0, 0};
    const uint32_t bpr = (r->tiles_x + 3) / 4, n_jobs = bpr * r->tiles_y;
    r->have_order = false;
    // (the order's slots come in groups of the tiles a wave of the pass will shade: launch_shade's rule)
    r->order_group = r->tiles_per_wave ? r->tiles_per_wave : ((uint32_t)r->n_tiles() < SMALL_FRAME_TILES ? 1u : DEFAULT_TILES_PER_WAVE);
    r->order_slots = order_slots(r->tiles_x, r->tiles_y, r->order_group);
    if (r->tile_order && n_jobs) {
        HIPCHECK(r, r->d_tile_class.ensure(r->n_tiles()));
        HIPCHECK(r, r->d_order_lists.ensure((size_t)n_jobs * 8));
        HIPCHECK(r, r->d_tile_order.ensure((size_t)r->order_slots * 4));
        hint.tile_class = r->d_tile_class.as<uint8_t>();
        hint.sky = r->env_w ? 1u : 0u;
        const uint32_t nb = shadow_bounds_pitch(r->shadow_size);
        if (nb && !(r->debug & 8)) {
            int rc = build_shadow_bounds(r, r->stream);
            if (rc != ARCTIC_OK) return rc;
            hint.bounds = r->d_shadow_bounds().as<float2>(); hint.S = r->shadow_size; hint.pitch = nb;
        }
    }
    r->lod_valid = false;
    if (r->texture_mips) {   // ... with the level-of-detail plane next to it (k_resolve_lod)
        HIPCHECK(r, r->d_lod.ensure(r->n_tiles() * TILE_PIXELS * 4));
        HIPCHECK(r, launch_resolve_lod(r->d_vis().as<unsigned long long>(), r->geo[r->fwd()].d_recs.as<SetupRec>(), r->geo[r->fwd()].d_rrecs.as<RasterRec>(), r->geo[r->fwd()].d_rec_of.as<uint32_t>(), r->tables[r->fwd()].objs,
                                       r->geo[r->fwd()].d_xverts.as<XVert>(), r->tables[r->fwd()].gp, (uint32_t)r->n_tiles(), r->gbuffer(), hint,
                                       r->d_tex.as<TexDesc>(), (uint32_t)(r->tex.size() / 3), r->d_lod.as<float>(), r->stream));
        r->lod_valid = true;
    } else
    HIPCHECK(r, launch_resolve(r->d_vis().as<unsigned long long>(), r->geo[r->fwd()].d_recs.as<SetupRec>(), r->geo[r->fwd()].d_rrecs.as<RasterRec>(), r->geo[r->fwd()].d_rec_of.as<uint32_t>(), r->tables[r->fwd()].objs,
                               r->geo[r->fwd()].d_xverts.as<XVert>(), r->tables[r->fwd()].gp, (uint32_t)r->n_tiles(), r->gbuffer(), hint,
                               r->stream));
    if (hint.tile_class) {
        HIPCHECK(r, launch_tile_order(hint.tile_class, r->tiles_x, r->tiles_y, r->order_tail, r->order_group, r->d_order_lists.as<uint32_t>(), r->d_tile_order.as<uint32_t>(), r->stream));
        r->have_order = true;
    }
    r->have_gbuffer = true;
    return ARCTIC_OK;
}
}  // namespace arctic
namespace {

int pass_gbuffer(ArcticRenderer *r, const ArcticScene *sc) {
    int rc = pass_visibility(r, sc, r->stream);
    return rc != ARCTIC_OK ? rc : resolve_gbuffer(r);
}

// the image-based ambient's tables from the map in d_env, in stream order on the handle's stream (arctic_create_hdri / arctic_set_option)
int build_env_tables(ArcticRenderer *r) {
    const uint32_t W = r->env_w, H = r->env_h;
    HIPCHECK(r, r->d_env_levels.ensure(env_levels_bytes(W, H)));
    HIPCHECK(r, r->d_env_lut.ensure((size_t)ENV_LUT * ENV_LUT * sizeof(float2)));
    HIPCHECK(r, r->d_env_mips.ensure(env_mips_bytes(W, H)));
    HIPCHECK(r, r->d_env_sh_rows.ensure((size_t)H * 27 * sizeof(double)));
    HIPCHECK(r, r->d_env_tables.ensure(sizeof(EnvTables)));
    EnvTables &T = r->env_host;
    T = EnvTables{};
    T.n_levels = ENV_LEVELS; T.lut_n = ENV_LUT;
    T.level[0] = r->d_env.as<float4>(); T.w[0] = W; T.h[0] = H;
    float4 *lv = r->d_env_levels.as<float4>();
    for (uint32_t k = 1; k < ENV_LEVELS; ++k) {
        env_level_size(W, H, k, T.w[k], T.h[k]);
        T.level[k] = lv; lv += (size_t)T.w[k] * T.h[k];
    }
    T.lut = r->d_env_lut.as<float2>();
    // (the struct goes up in stream order too: the kernels below write its sh[] behind the copy; a pageable source is staged by HIP before the call returns)
    HIPCHECK(r, hipMemcpyAsync(r->d_env_tables.p, &T, sizeof T, hipMemcpyHostToDevice, r->stream));
    EnvBuild b = {r->d_env.as<float4>(), W, H, r->d_env_levels.as<float4>(), r->d_env_lut.as<float2>(), r->d_env_mips.as<float4>(),
                  r->d_env_sh_rows.as<double>(), r->d_env_tables.as<EnvTables>()};
    HIPCHECK(r, launch_env_build(b, r->stream));
    r->env_built = true;
    return ARCTIC_OK;
}

int fill_shade_params(ArcticRenderer *r, const ArcticScene *sc, const ArcticSettings *st, void *d_out, ShadeParams &sp, bool from_vis = false) {
    if (!from_vis && !r->have_gbuffer) {
        if (r->have_vis) { int rc = resolve_gbuffer(r); if (rc != ARCTIC_OK) return rc; }   // frame came from arctic_render_frame
        else return r->fail(ARCTIC_E_STATE, "shade: no G-buffer (run arctic_pass_gbuffer or arctic_write_gbuffer first)");
    }
    if (r->mips_active() && (r->count_evals || r->tile_trace))
        return r->fail(ARCTIC_E_STATE, "shade: ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE do not apply to mip-mapped material textures (ARCTIC_OPT_TEXTURE_MIPS = 1 with a chain)");
    if (!from_vis && r->mips_active() && !r->lod_valid) {   // the G-buffer in place was made with the option off: its plane from the visibility, or zeroes
        if (r->have_vis) { int rc = resolve_gbuffer(r); if (rc != ARCTIC_OK) return rc; }
        else {
            HIPCHECK(r, r->d_lod.ensure(r->n_tiles() * TILE_PIXELS * 4));
            HIPCHECK(r, hipMemsetAsync(r->d_lod.p, 0, r->n_tiles() * TILE_PIXELS * 4, r->stream));
            r->lod_valid = true;
        }
    }
    if (r->env_active() && (r->count_evals || r->tile_trace))
        return r->fail(ARCTIC_E_STATE, "shade: ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE do not apply to the image-based ambient (ARCTIC_OPT_ENV_LIGHTING = 1 with a map)");
    if (r->n_spots && (r->count_evals || r->tile_trace))
        return r->fail(ARCTIC_E_STATE, "shade: ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE do not apply with spot lights (arctic_update_spot_lights)");
    if (r->n_cubes && (r->count_evals || r->tile_trace))
        return r->fail(ARCTIC_E_STATE, "shade: ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE do not apply with shadow-casting point lights (arctic_update_point_shadow_lights)");
    if (r->has_extras() && (r->count_evals || r->tile_trace))
        return r->fail(ARCTIC_E_STATE, "shade: ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE do not apply while a material has extras (arctic_set_material_extras)");
    std::memset(&sp, 0, sizeof sp);
    sp.g = r->gbuffer();
    const ArcticRenderer::GeoSet &G = r->geo[r->fwd()];
    sp.compact_tables = (G.d_recs.cap < (1ull << 32) && G.d_rrecs.cap < (1ull << 32) && G.d_xverts.cap < (1ull << 32) && G.d_rec_of.cap < (1ull << 32) &&
                         r->tables[r->fwd()].d.cap < (1ull << 32) && !(r->debug & 64)) ? 1 : 0;
    sp.vis = r->d_vis().as<unsigned long long>();
    if (!from_vis && r->mips_active()) sp.lod = r->d_lod.as<float>();   // (k_miplit: the G-buffer walk reads no visibility plane, the plane takes its slot)
    sp.recs = G.d_recs.as<SetupRec>(); sp.rrecs = G.d_rrecs.as<RasterRec>(); sp.rec_of = G.d_rec_of.as<uint32_t>();
    sp.objs = r->tables[r->fwd()].objs; sp.xv = G.d_xverts.as<XVert>();
    sp.tex = r->d_tex.as<TexDesc>();
    sp.n_materials = (uint32_t)(r->tex.size() / 3);
    sp.srgb_lut = r->d_lut.as<float>();
    sp.shadow_map = r->shadow_size ? r->d_shadow().as<float>() : nullptr;
    sp.shadow_size = r->shadow_size;
    sp.lights = r->d_lights.as<float4>(); sp.light_pairs = r->d_light_pairs.as<float4>();
    sp.n_lights = r->n_lights; sp.pair_runs = r->pair_runs;
    std::memcpy(sp.eye, sc->camera.eye, 12);
    dir_from_rot(sc->sun.rotation, sp.sun_dir);     // DirectionalLight::direction(), scene.cpp:56-59
    std::memcpy(sp.sun_color, sc->sun.color, 12);
    sp.ambient = sc->ambient;
    sp.tm_method = st->tm_method;
    sp.inv_gamma = 1.0f / st->gamma;
    sp.exposure = st->exposure;
    sp.width = r->width; sp.rows = r->rows(); sp.row0_in_tile = r->row0_in_tile;
    sp.tiles_x = r->tiles_x; sp.tiles_y = r->tiles_y;
    sp.out_rgba8 = static_cast<uint8_t *>(d_out && !r->aa_active() ? d_out : r->d_rgba8.p);   // (with the edge filter: always the handle's own, the filter writes d_out)
    size_t out_px = (size_t)r->rows() * r->width;
    if (r->keep_float) {
        HIPCHECK(r, r->d_ldr.ensure(out_px * 12));
        HIPCHECK(r, r->d_hdr.ensure(out_px * 12));
        sp.out_ldr = r->d_ldr.as<float>(); sp.out_hdr = r->d_hdr.as<float>();
    }
    sp.stats = nullptr;
    sp.trace = nullptr;
    if (r->tile_trace) {
        const size_t bytes = (size_t)r->tiles_x * r->tiles_y * 32;
        HIPCHECK(r, r->d_tile_trace.ensure(bytes));
        HIPCHECK(r, hipMemsetAsync(r->d_tile_trace.p, 0, bytes, r->stream));
        sp.trace = r->d_tile_trace.as<unsigned long long>();
    }
    if (r->n_spots) { sp.spots = r->d_spots.as<float4>(); sp.n_spots = r->n_spots; }   // (the statistics' slot: k_spotlit* keep none)
    if (r->n_cubes) { sp.cubes = r->d_cubes.as<float4>(); sp.n_cubes = r->n_cubes; sp.cube_size = r->cube_size; }   // (the trace's slot: k_cubelit* keep none)
    // (the order was built for groups of order_group tiles per wave: a pass that shades another number per wave takes the geometric order)
    if (r->env_active()) sp.env_tables = r->d_env_tables.as<EnvTables>();   // (the geometric order: the tables take the order's slot)
    else if (r->n_spots || r->n_cubes || r->mips_active() || r->has_extras()) {}                                    // (k_spotlit*, k_cubelit*: the geometric order)
    else if (!from_vis && r->have_order && r->tile_order && (r->tiles_per_wave == 0 || r->tiles_per_wave == r->order_group)) {
        sp.tile_order = r->d_tile_order.as<uint32_t>(); sp.n_jobs = r->order_slots; sp.tiles_per_wave = r->order_group;
    }
    sp.culling = r->culling;
    sp.debug = r->debug | (sp.trace ? (1 << 30) : 0) | ((r->sampler & 5) << 20);   // bit 30: the kernels learn of the trace from the first block of their arguments; bits 20..22: ARCTIC_OPT_SAMPLER (shade.hip SAMPLER_SHIFT)
    sp.hdr16 = r->hdr16;
    sp.env = r->env_w ? r->d_env.as<float4>() : nullptr; sp.env_w = r->env_w; sp.env_h = r->env_h;
    camera_sky_basis(sc->camera.rotation, sc->camera.aspect, sc->camera.fov_y, sp.sky_fwd, sp.sky_right, sp.sky_up);
    sp.ndc_sx = 2.0f / (float)r->width; sp.ndc_sy = 2.0f / (float)r->height;
    sp.band_tiles = (int32_t)(r->band_rows / TILE); sp.shard_index = (int32_t)r->shard_index; sp.shard_count = (int32_t)r->shard_count;
    sp.tile_y0 = (int32_t)r->tile_y0;
    const uint32_t nb = shadow_bounds_pitch(r->shadow_size);
    if (nb && !(r->debug & 8)) {   // the min/max table of the shadow map: rebuilt whenever the map was written
        int rc = build_shadow_bounds(r, r->stream);
        if (rc != ARCTIC_OK) return rc;
        sp.shadow_bounds = r->d_shadow_bounds().as<float2>(); sp.bounds_pitch = nb;
    }
    return ARCTIC_OK;
}

// one shading pass = one launch.  The light loop: scalar up to 12 point lights, packed pairs above (both read the lights through the scalar
// cache; measured crossover, profiles/r3_light_paths.txt: 8 lights 0.1062 / 0.1072 ms, 12: 0.1125 / 0.1138, 16: 0.123 / 0.1186;
// ARCTIC_OPT_LIGHT_PATH overrides).
hipError_t shade_once(ArcticRenderer *r, const ShadeParams &sp, bool from_vis, bool stats) {
    ShadeLaunch L;
    L.stream = r->stream;
    L.loop = r->light_path == 0 ? (sp.n_lights <= 12 ? 1u : 2u) : (uint32_t)r->light_path;
    L.from_vis = from_vis ? 1u : 0u;
    L.stats = stats ? 1u : 0u;
    L.tiles_per_wave = r->tiles_per_wave;
    L.env = r->env_active() ? 1u : 0u;
    L.spot = sp.n_spots ? 1u : 0u;
    L.cube = sp.n_cubes ? 1u : 0u;
    L.mip = r->mips_active() ? 1u : 0u;
    L.pbr = r->has_extras() ? 1u : 0u;
    return launch_shade(sp, L);
}

int pass_shade(ArcticRenderer *r, const ArcticScene *sc, const ArcticSettings *st, void *d_out, bool from_vis = false) {
    Range zone("Forward Pass: shading + Skybox Pass + Post Process Pass");
    ShadeParams sp;
    int rc = fill_shade_params(r, sc, st, d_out, sp, from_vis);
    if (rc != ARCTIC_OK) return rc;
    // ARCTIC_OPT_ANTIALIAS: the shading kernels write d_rgba8, the filter the destination
    const bool aa = r->aa_active();
    void *aa_out = nullptr;
    if (aa) {
        if (!d_out) HIPCHECK(r, r->d_aa.ensure((size_t)r->rows() * r->width * 4));
        aa_out = d_out ? d_out : r->d_aa.p;
    }
    HIPCHECK(r, r->shard_readers.wait_for(sp.out_rgba8, r->stream));   // a gather of an earlier frame may still be reading this output buffer ...
    HIPCHECK(r, r->shard_readers.wait_for(aa_out, r->stream));         // ... or the one the filter writes
    if (r->count_evals) {
        sp.stats = r->d_counter.as<unsigned long long>();
        HIPCHECK(r, hipMemsetAsync(r->d_counter.p, 0, 8 * N_SHADE_STATS, r->stream));
    }
    HIPCHECK(r, shade_once(r, sp, from_vis, r->count_evals != 0));
    if (aa) {
        Range aa_zone("Anti-aliasing Pass");
        HIPCHECK(r, launch_antialias(r->d_rgba8.p, aa_out, r->width, r->rows(), r->stream));
    }
    if (r->count_evals) {
        unsigned long long n[N_SHADE_STATS] = {};
        HIPCHECK(r, hipMemcpyAsync(n, r->d_counter.p, 8 * N_SHADE_STATS, hipMemcpyDeviceToHost, r->stream));
        HIPCHECK(r, hipStreamSynchronize(r->stream));
        r->stats[5] = n[0]; r->stats[6] = n[1]; r->stats[7] = n[2];
        r->light_stats[0] = n[3]; r->light_stats[1] = n[4]; r->stats[4] = n[9];
        for (int i = 0; i < 4; ++i) r->edge_stats[i] = n[5 + i];
    }
    r->have_output = (d_out == nullptr);
    r->hdr_valid = r->keep_float != 0;   // (sp.out_hdr: this pass wrote d_hdr, or it did not)
    r->output_filtered = aa && d_out == nullptr;
    return ARCTIC_OK;
}

}  // namespace
namespace arctic {   // (renderer_state.h: other units call it)
// the tail of every cache key (shadow_inputs, cube_inputs, ray_inputs): per object its transform, its mesh and -- the mesh exists -- the mesh's
// shape: a skin, pose or morph call changes what the object casts (arctic_set_mesh_pose)
void put_objects(const ArcticRenderer *r, const ArcticScene *sc, std::vector<uint8_t> &k) {
    auto put = [&](const void *p, size_t n) { const uint8_t *b = static_cast<const uint8_t *>(p); k.insert(k.end(), b, b + n); };
    for (uint64_t i = 0; i < sc->n_objects; ++i) {
        put(sc->objects[i].trs, sizeof sc->objects[i].trs); put(&sc->objects[i].mesh_idx, sizeof sc->objects[i].mesh_idx);
        if (sc->objects[i].mesh_idx < r->meshes.size()) put(&r->meshes[sc->objects[i].mesh_idx].shape_seq, sizeof(uint64_t));
    }
}
}  // namespace arctic
namespace {

// everything the shadow map is a function of, as bytes (compared exactly, not hashed)
std::vector<uint8_t> shadow_inputs(const ArcticRenderer *r, const ArcticScene *sc) {
    std::vector<uint8_t> k;
    if (!r->shadow_size) return k;
    auto put = [&](const void *p, size_t n) { const uint8_t *b = static_cast<const uint8_t *>(p); k.insert(k.end(), b, b + n); };
    const uint64_t head[3] = {r->shadow_size, (uint64_t)r->meshes.size(), sc->n_objects};
    put(head, sizeof head);
    put(sc->sun.position, sizeof sc->sun.position);
    put(sc->sun.rotation, sizeof sc->sun.rotation);
    put_objects(r, sc, k);
    return k;
}

// everything the point lights' faces are a function of, as bytes (shadow_inputs' rule)
std::vector<uint8_t> cube_inputs(const ArcticRenderer *r, const ArcticScene *sc) {
    std::vector<uint8_t> k;
    if (!r->n_cubes) return k;
    auto put = [&](const void *p, size_t n) { const uint8_t *b = static_cast<const uint8_t *>(p); k.insert(k.end(), b, b + n); };
    const uint64_t head[6] = {r->cube_size, r->n_cubes, (uint64_t)r->meshes.size(), sc->n_objects, (uint64_t)r->cluster_cull, (uint64_t)r->small_triangles};
    put(head, sizeof head);
    put(r->cube_lights.data(), r->cube_lights.size() * sizeof(ArcticPointShadowLight));
    put_objects(r, sc, k);
    return k;
}

// a stream other than the main one is about to run a prepass: it first waits for the latest k_skin (enqueued on the main stream)
int wait_skin(ArcticRenderer *r, hipStream_t stream, uint64_t &seen) {
    HIPCHECK(r, r->deformed.wait_once(stream, seen));
    return ARCTIC_OK;
}

}  // namespace
namespace arctic {   // (renderer_state.h: other units call it)
// after a stream synchronisation: did a rasteriser pass run out of work-item slots?  (k_setup flags it; the table is re-sized
// from the counts of that very pass, so rendering the frame again succeeds)
int check_item_overflow(ArcticRenderer *r) {
    bool cube_overflow = false;   // a face of a point light (pass_point_shadows: its own slots)
    uint32_t need = 0;
    for (uint32_t j = 0; r->h_cube_counts() && j < r->n_cubes * 6; ++j) {
        uint32_t *c = r->h_cube_counts() + CUBE_COUNT_WORDS * j;
        if (c[2]) { cube_overflow = true; need = std::max(need, c[1]); c[2] = 0; }
    }
    if (cube_overflow) r->cube_key.clear();
    if (!r->h_counts() || !(r->h_counts()[4] | r->h_counts()[5] | (cube_overflow ? 1u : 0u))) return ARCTIC_OK;
    need = std::max(need, std::max(r->h_counts()[1], r->h_counts()[3]));
    r->h_counts()[4] = r->h_counts()[5] = 0;
    r->recs_worst_case = true;   // whichever table it was: the record table takes its worst-case size from now on
    r->have_gbuffer = false; r->have_output = false; r->hdr_valid = false; r->have_vis = false; r->have_order = false; r->shadow_key.clear();
    return r->fail(ARCTIC_E_CAPACITY, "a rasteriser table overflowed (%u work items needed, %u slots; or more than 2 records per source triangle): the last frame "
                   "is incomplete; the tables grow on the next pass -- render the frame again", need, std::max(r->geo[0].item_cap, r->geo[1].item_cap));
}
}  // namespace arctic
namespace {

// The device's texture table: the 3 * n_materials descriptors and, while a material has extras, one MaterialExtra per material behind them
// (common.h).  Uploaded whenever either part changes; the caller has drained the stream.
int upload_tex_table(ArcticRenderer *r) {
    const size_t n = r->tex.size() / 3, desc_bytes = r->tex.size() * sizeof(TexDesc);
    std::vector<char> table(desc_bytes + (r->has_extras() ? n * sizeof(MaterialExtra) : 0));
    std::memcpy(table.data(), r->tex.data(), desc_bytes);
    for (size_t m = 0; r->has_extras() && m < n; ++m) {
        const ArcticRenderer::Extras &x = r->extras[m];
        MaterialExtra e = {};
        std::memcpy(&e.base_color[0], x.p, 10 * sizeof(float));   // base_color .. emissive2 are the first ten floats of both
        if (x.d_fast) {
            const uint32_t w = r->tex[3 * m].w & ~TEX_INTERLEAVED, h = r->tex[3 * m].h;
            e.flags = EXTRA_FAST | (x.ew ? EXTRA_EMISSIVE : 0u) | (x.ow ? EXTRA_OCCLUSION : 0u);
            e.emissive = TexDesc{x.d_fast.as<const uint32_t>(), w, h, (float)w, (float)h, w + 2, 0u};
        } else {
            if (x.d_emissive) { e.flags |= EXTRA_EMISSIVE; e.emissive = TexDesc{x.d_emissive.as<const uint32_t>(), x.ew, x.eh, (float)x.ew, (float)x.eh, x.ew, 0u}; }
            if (x.d_occlusion) { e.flags |= EXTRA_OCCLUSION; e.occlusion = TexDesc{x.d_occlusion.as<const uint32_t>(), x.ow, x.oh, (float)x.ow, (float)x.oh, x.ow, 0u}; }
        }
        std::memcpy(table.data() + desc_bytes + m * sizeof(MaterialExtra), &e, sizeof e);
    }
    HIPCHECK(r, r->d_tex.ensure(std::max<size_t>(48, table.size())));
    if (!table.empty()) HIPCHECK(r, hipMemcpy(r->d_tex.p, table.data(), table.size(), hipMemcpyHostToDevice));
    return ARCTIC_OK;
}

}  // namespace
namespace arctic {   // (renderer_state.h: other units call it)
bool valid_scene(const ArcticScene *sc) { return sc && (sc->n_objects == 0 || sc->objects); }
}  // namespace arctic

// =================================================================================================
extern "C" {

int arctic_version(void) { return 340; }

ArcticRenderer *arctic_create(const ArcticCreateInfo *info, char *err, uint64_t err_len) {
    auto say = [&](const char *m) { if (err && err_len) { std::snprintf(err, (size_t)err_len, "%s", m); } };
    if (!info || info->width == 0 || info->height == 0) { say("arctic_create: width/height must be > 0"); return nullptr; }
    if (info->width > MAX_TARGET || info->height > MAX_TARGET || info->shadow_size > MAX_TARGET) { say("arctic_create: targets above 16384 pixels a side are not supported"); return nullptr; }
    uint32_t rb = info->row_begin, re = info->row_end;
    if (rb == 0 && re == 0) re = info->height;
    if (re > info->height || rb >= re) { say("arctic_create: bad row shard"); return nullptr; }
    if (info->band_rows) {
        if (info->band_rows % TILE != 0 || info->shard_count == 0 || info->shard_index >= info->shard_count || info->row_begin || info->row_end) {
            say("arctic_create: bad interleaved shard (band_rows must be a multiple of 8, shard_index < shard_count, row_begin = row_end = 0)");
            return nullptr;
        }
        if ((uint64_t)info->shard_index * info->band_rows >= info->height) { say("arctic_create: interleaved shard owns no rows"); return nullptr; }
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { say("arctic_create: no HIP device (this library has no CPU path)"); return nullptr; }
    if (info->device < 0 || info->device >= n_dev) { say("arctic_create: device ordinal out of range"); return nullptr; }
    ArcticRenderer *r = new ArcticRenderer();
    r->device = info->device;
    r->width = info->width; r->height = info->height; r->shadow_size = info->shadow_size; r->max_lights = info->max_lights;
    r->row_begin = rb; r->row_end = re;
    r->band_rows = info->band_rows; r->shard_index = info->shard_index; r->shard_count = info->band_rows ? info->shard_count : 1;
    auto bail = [&](const char *what, hipError_t e) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "arctic_create: %s: %s", what, hipGetErrorString(e));
        say(buf);
        arctic_destroy(r);
        return (ArcticRenderer *)nullptr;
    };
    hipError_t e;
    // The events below order streams of THIS device among each other (prepass / shadow pass / shading of frames in flight); nothing waits for them on the
    // host or on another device.  Without the system-scope fence HIP otherwise puts around every record and wait -- a cache write-back and invalidate between
    // two shading kernels -- a 4K frame takes 0.256 instead of 0.261 ms, one rank of 8's 0.065 instead of 0.069 (round 5, tools/experiments/cull_ab.py's loop).
    // (`shaded` and the gather's marks, which RCCL's transfers to other devices follow, keep the default.)
    const unsigned in_device_event = hipEventDisableTiming | hipEventDisableSystemFence;
    if ((e = hipSetDevice(r->device)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = r->own_stream.create(hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    r->stream = r->own_stream;
    if ((e = r->shadow_stream.create(hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = r->shadow_fork.create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = r->shadow_drawn.create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = r->shadow_scratch_free.create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = r->deformed.create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    // The HIP runtime deals its hardware queues (4 by default, GPU_MAX_HW_QUEUES) to streams in the order they are created, and two
    // streams on one queue do not overlap: the handle's own stream, the shadow stream and the first prepass stream are created here, in
    // that order (with a caller's stream that makes four); the second prepass stream, which only three frames in flight use, is the
    // handle's own stream when the caller brought one (it is idle then), else created when first needed (second_prepass_stream)
    if ((e = r->prepass_stream[0].create(hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    for (int k = 0; k < 2; ++k)
        if ((e = r->prepass_done[k].create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    for (StreamMark &m : r->vis_set_released)
        if ((e = m.create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    for (StreamMark &m : r->shadow_set_released)
        if ((e = m.create(in_device_event)) != hipSuccess) return bail("hipEventCreate", e);
    {
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, r->device)) != hipSuccess) return bail("hipGetDeviceProperties", e);
        r->cu_count = (uint32_t)std::max(1, prop.multiProcessorCount);
        r->raster_blocks[0] = raster_grid_blocks(false, r->cu_count);
        r->raster_blocks[1] = raster_grid_blocks(true, r->cu_count);
        if ((e = r->counts.alloc(64, hipHostMallocMapped)) != hipSuccess) return bail("hipHostMalloc", e);
        std::memset(r->h_counts(), 0, 64);
    }
    float lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = srgb8_to_linear(i);
    if ((e = r->d_lut.ensure(sizeof lut)) != hipSuccess) return bail("hipMalloc lut", e);
    if ((e = hipMemcpy(r->d_lut.p, lut, sizeof lut, hipMemcpyHostToDevice)) != hipSuccess) return bail("upload lut", e);
    if ((e = r->d_lights.ensure(std::max<size_t>(32, (size_t)r->max_lights * 32))) != hipSuccess) return bail("hipMalloc lights", e);
    if ((e = r->d_light_pairs.ensure(std::max<size_t>(48, (size_t)((r->max_lights + 1) / 2) * 48))) != hipSuccess) return bail("hipMalloc light pairs", e);
    if ((e = r->d_tex.ensure(48)) != hipSuccess) return bail("hipMalloc tex table", e);
    if (r->shadow_size) {
        size_t n = (size_t)r->shadow_size * r->shadow_size;
        if ((e = r->d_shadow().ensure(shadow_alloc_bytes(r))) != hipSuccess) return bail("hipMalloc shadow map", e);
        if ((e = launch_fill_u32(r->d_shadow().as<uint32_t>(), 0x3F800000u, n, r->stream)) != hipSuccess) return bail("clear shadow map", e);
    }
    if (alloc_targets(r) != ARCTIC_OK) { say(r->err.c_str()); arctic_destroy(r); return nullptr; }
    if ((e = hipStreamSynchronize(r->stream)) != hipSuccess) return bail("sync", e);
    return r;
}

// Nothing is released by name here: once the streams are idle the handle's members release themselves (device_resources.h), the streams first
// (ArcticRenderer declares them last).
void arctic_destroy(ArcticRenderer *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    if (r->shadow_stream) (void)hipStreamSynchronize(r->shadow_stream);
    for (hipStream_t ps : r->prepass_stream) if (ps) (void)hipStreamSynchronize(ps);
    if (r->own_stream) (void)hipStreamSynchronize(r->own_stream);
    (void)arctic_comm_destroy(r);
    delete r;
}

const char *arctic_last_error(const ArcticRenderer *r) { return r ? r->err.c_str() : "null handle"; }

int arctic_resize(ArcticRenderer *r, uint32_t width, uint32_t height) {
    if (!r) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0) return r->fail(ARCTIC_E_INVALID, "resize: zero size");
    if (width > MAX_TARGET || height > MAX_TARGET) return r->fail(ARCTIC_E_CAPACITY, "resize: targets above 16384 pixels a side are not supported");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    r->width = width; r->height = height; r->row_begin = 0; r->row_end = height;
    r->band_rows = 0; r->shard_index = 0; r->shard_count = 1;
    return alloc_targets(r);
}

namespace {
// the main stream and whatever runs prepasses for it: what arctic_flush and a change of the frames in flight wait for
int drain_frame_streams(ArcticRenderer *r) {
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    for (hipStream_t ps : r->prepass_stream) if (ps) HIPCHECK(r, hipStreamSynchronize(ps));   // (joined into the main stream by every frame; after a failed frame they may not be)
    if (r->own_stream_is_prepass()) HIPCHECK(r, hipStreamSynchronize(r->own_stream));         // (the second prepass stream of a handle on a caller's stream)
    return ARCTIC_OK;
}
}  // namespace

int arctic_flush(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = select_device(r);
    if (rc) return rc;
    if ((rc = drain_frame_streams(r)) != ARCTIC_OK) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->shadow_stream));
    if (r->comm_stream) HIPCHECK(r, hipStreamSynchronize(r->comm_stream));
    if (int ov = check_item_overflow(r)) return ov;
    return ARCTIC_OK;
}

int arctic_set_stream(ArcticRenderer *r, void *hip_stream) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    // (own_stream may be the second prepass stream of the frames in flight; when it carries the exchange instead -- borrowed as the
    //  communication stream -- it is NOT waited for here: it may hold a collective the other ranks have not reached yet)
    if (r->own_stream_is_prepass()) HIPCHECK(r, hipStreamSynchronize(r->own_stream));
    r->stream = static_cast<hipStream_t>(hip_stream);   // NULL = the default stream
    r->skin_seen_prepass[1] = 0;   // (the second prepass stream may be another one now: it waits for the latest k_skin again)
    return ARCTIC_OK;
}

int arctic_use_own_stream(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (r->own_stream_is_prepass()) HIPCHECK(r, hipStreamSynchronize(r->own_stream));
    if (r->comm_stream_borrowed) {
        // One role per stream.  The exchange KEEPS the stream it has been running on -- it may hold gathers the other ranks have not matched yet, and
        // passes queued behind those would stall until they do -- and becomes its owner; the passes get a fresh stream (ordered against earlier
        // gathers the way they always are: by the events of the shard buffers they write, pass_shade).  The new stream goes into a local first: a
        // failed creation leaves the handle exactly as it was.
        Stream fresh;
        HIPCHECK(r, fresh.create(hipStreamNonBlocking));
        r->comm_stream_borrowed = false;   // comm_stream == the old own_stream: owned by the exchange from here on (destroyed with the communicator)
        r->comm_stream_owned = std::move(r->own_stream);
        r->own_stream = std::move(fresh);
    }
    r->stream = r->own_stream;
    r->skin_seen_prepass[1] = 0;
    return ARCTIC_OK;
}

int arctic_create_material(ArcticRenderer *r, const void *diffuse, uint32_t dw, uint32_t dh, const void *normal, uint32_t nw,
                           uint32_t nh, const void *mr, uint32_t mw, uint32_t mh) {
    if (!r) return ARCTIC_E_INVALID;
    if (!diffuse || !normal || !mr || !dw || !dh || !nw || !nh || !mw || !mh) return r->fail(ARCTIC_E_INVALID, "create_material: null image or zero size");
    if ((dw | dh | nw | nh | mw | mh) & 0xFFFF0000u) return r->fail(ARCTIC_E_CAPACITY, "create_material: image side above 65535");
    int rc = select_device(r);
    if (rc) return rc;
    const void *src[3] = {diffuse, normal, mr};
    const uint32_t w[3] = {dw, nw, mw}, h[3] = {dh, nh, mh};
    TexDesc td[3];
    std::vector<TexDesc> chain;   // ARCTIC_OPT_TEXTURE_MIPS: one descriptor per level; empty: one level
    // byte offsets into an image are 32-bit in the kernels (shade.hip: saddr loads)
    if ((uint64_t)(dw + 2) * (dh + 2) > (1ull << 29) || (uint64_t)nw * nh > (1ull << 30) || (uint64_t)mw * mh > (1ull << 30))
        return r->fail(ARCTIC_E_CAPACITY, "create_material: image above 2^29 texels");
    if (dw == nw && dw == mw && dh == nh && dh == mh) {
        // equal sizes (the usual glTF case): pack the eight channels ps_main reads into 8-byte texels, with a one-texel WRAP
        // border around the image (layout: common.h TexDesc, shade.hip)
        const uint32_t pw = dw + 2, ph = dh + 2;
        // 4 x 4-texel tiles for textures that will be minified at their only mip level (common.h TexDesc::tile_row_bytes): the library's choice is by
        // size -- a 2048^2 image on a model that covers a part of a 1080p or 4K frame is sampled several texels apart, a 1024^2 wall texture about 1:1,
        // where the row-major strips of neighbouring pixels share their lines and the tiled address (15 instructions against 3) would only cost
        const bool tiled = r->texture_tiling < 0 ? std::min(dw, dh) >= 2048u : r->texture_tiling != 0;
        const uint32_t tpr = (pw + 3) / 4, trows = (ph + 3) / 4;
        size_t n = tiled ? (size_t)tpr * trows * 16 : (size_t)pw * ph;
        if (n > (1ull << 29)) return r->fail(ARCTIC_E_CAPACITY, "create_material: image above 2^29 texels");
        // ARCTIC_OPT_TEXTURE_MIPS: the chain behind level 0 in the same allocation (common.h), levels 1.. row-major with their own border, at
        // 256-byte aligned offsets; the whole of it below 2^32 bytes (checked before anything is allocated: the handle stays as it was)
        const uint32_t levels = r->texture_mips ? mip_level_count(dw, dh) : 1u;
        std::vector<uint64_t> level_offset(levels, 0);
        uint64_t chain_bytes = (uint64_t)n * 8;
        for (uint32_t k = 1; k < levels; ++k) {
            chain_bytes = (chain_bytes + 255) & ~255ull;
            level_offset[k] = chain_bytes;
            chain_bytes += (uint64_t)(mip_level_side(dw, k) + 2) * (mip_level_side(dh, k) + 2) * 8;
        }
        if (chain_bytes > (1ull << 32)) return r->fail(ARCTIC_E_CAPACITY, "create_material: the mip chain does not fit in 2^32 bytes (ARCTIC_OPT_TEXTURE_MIPS)");
        std::vector<uint32_t> packed(n * 2);
        const uint8_t *a = static_cast<const uint8_t *>(diffuse), *b = static_cast<const uint8_t *>(normal), *c = static_cast<const uint8_t *>(mr);
        for (uint32_t Y = 0; Y < ph; ++Y) {
            const size_t sy = (size_t)((Y + dh - 1) % dh) * dw;
            for (uint32_t X = 0; X < pw; ++X) {
                const size_t i = sy + (X + dw - 1) % dw;
                const size_t o = tiled ? ((size_t)(Y >> 2) * tpr + (X >> 2)) * 16 + (Y & 3) * 4 + (X & 3) : (size_t)Y * pw + X;
                packed[2 * o] = (uint32_t)a[4 * i] | ((uint32_t)a[4 * i + 1] << 8) | ((uint32_t)a[4 * i + 2] << 16) | ((uint32_t)b[4 * i] << 24);
                packed[2 * o + 1] = (uint32_t)b[4 * i + 1] | ((uint32_t)b[4 * i + 2] << 8) | ((uint32_t)c[4 * i + 1] << 16) | ((uint32_t)c[4 * i + 2] << 24);
            }
        }
        DevBuf image;
        HIPCHECK(r, image.alloc_exact((size_t)chain_bytes));
        void *const p = image.p;
        r->tex_allocs.push_back(std::move(image));
        HIPCHECK(r, hipMemcpy(p, packed.data(), n * 8, hipMemcpyHostToDevice));   // synchronous like rhi.cpp:480-519
        for (int i = 0; i < 3; ++i) { td[i] = TexDesc{static_cast<const uint32_t *>(p), dw | TEX_INTERLEAVED, dh, (float)dw, (float)dh, pw, tiled ? tpr * 128u : 0u}; }
        if (r->texture_mips) {   // level k + 1 from level k on the device (texture_mips.hip), synchronous like the upload; the material's table of levels
            chain.resize(levels);
            chain[0] = td[0];
            for (uint32_t k = 1; k < levels; ++k) {
                const uint32_t wk = mip_level_side(dw, k), hk = mip_level_side(dh, k);
                chain[k] = TexDesc{reinterpret_cast<const uint32_t *>(static_cast<const char *>(p) + level_offset[k]), wk | TEX_INTERLEAVED, hk, (float)wk, (float)hk, wk + 2, 0u};
                HIPCHECK(r, launch_mip_reduce(chain[k - 1], chain[k], r->d_lut.as<float>(), r->stream));
            }
            DevBuf levels_table;
            HIPCHECK(r, levels_table.alloc_exact(levels * sizeof(TexDesc)));
            void *const table = levels_table.p;
            r->tex_allocs.push_back(std::move(levels_table));
            HIPCHECK(r, hipMemcpyAsync(table, chain.data(), levels * sizeof(TexDesc), hipMemcpyHostToDevice, r->stream));
            HIPCHECK(r, hipStreamSynchronize(r->stream));
            td[1] = TexDesc{static_cast<const uint32_t *>(table), levels, 0u, 0.0f, 0.0f, 0u, 0u};   // the MipTable (common.h)
        }
    } else {
        for (int i = 0; i < 3; ++i) {
            size_t bytes = (size_t)w[i] * h[i] * 4;
            DevBuf image;
            HIPCHECK(r, image.alloc_exact(bytes));
            void *const p = image.p;
            r->tex_allocs.push_back(std::move(image));
            HIPCHECK(r, hipMemcpy(p, src[i], bytes, hipMemcpyHostToDevice));
            td[i] = TexDesc{static_cast<const uint32_t *>(p), w[i], h[i], (float)w[i], (float)h[i], w[i], 0u};
        }
    }
    r->tex.insert(r->tex.end(), td, td + 3);
    if (!chain.empty()) ++r->n_chains;
    r->chains.push_back(std::move(chain));
    r->extras.emplace_back();
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int up = upload_tex_table(r)) return up;
    return (int)(r->tex.size() / 3) - 1;
}

int arctic_check_material_params(const ArcticMaterialParams *params) {
    return params && material_params_valid(params->base_color_factor) ? ARCTIC_OK : ARCTIC_E_INVALID;
}

int arctic_set_material_extras(ArcticRenderer *r, uint64_t material, const ArcticMaterialParams *params, const void *emissive, uint32_t ew, uint32_t eh,
                               const void *occlusion, uint32_t ow, uint32_t oh) {
    if (!r) return ARCTIC_E_INVALID;
    if (material >= r->tex.size() / 3) return r->fail(ARCTIC_E_INVALID, "set_material_extras: material %llu does not exist", (unsigned long long)material);
    if (params && arctic_check_material_params(params) != ARCTIC_OK)
        return r->fail(ARCTIC_E_INVALID, "set_material_extras: a field out of range or not finite, or a non-zero reserved field");
    if ((emissive != nullptr) != (ew != 0 && eh != 0) || (!emissive && (ew | eh)) || (occlusion != nullptr) != (ow != 0 && oh != 0) || (!occlusion && (ow | oh)))
        return r->fail(ARCTIC_E_INVALID, "set_material_extras: an image with a side of 0, or a size without an image");
    if ((ew | eh | ow | oh) & 0xFFFF0000u) return r->fail(ARCTIC_E_CAPACITY, "set_material_extras: image side above 65535");
    if ((uint64_t)ew * eh > (1ull << 30) || (uint64_t)ow * oh > (1ull << 30)) return r->fail(ARCTIC_E_CAPACITY, "set_material_extras: image above 2^30 texels");
    int rc = select_device(r);
    if (rc) return rc;
    ArcticRenderer::Extras nx;
    if (params) std::memcpy(nx.p, params->base_color_factor, sizeof nx.p);
    nx.ew = ew; nx.eh = eh; nx.ow = ow; nx.oh = oh;
    const ArcticRenderer::Extras neutral;
    nx.neutral = !emissive && !occlusion && std::memcmp(nx.p, neutral.p, sizeof nx.p) == 0;
    // the new images first: a failed allocation leaves the material as it was
    const TexDesc &d0 = r->tex[3 * material];
    const uint32_t mw = d0.w & ~TEX_INTERLEAVED, mh = d0.h;
    const bool fast = (d0.w & TEX_INTERLEAVED) && (emissive || occlusion) && (!emissive || (ew == mw && eh == mh)) && (!occlusion || (ow == mw && oh == mh));
    const auto upload = [&](DevBuf &dst, const void *src, size_t bytes) {
        return dst.alloc_exact(bytes) == hipSuccess && hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    bool ok = true;
    if (fast) {   // one image of 4-byte texels {e.r, e.g, e.b, o} with the packed image's one-texel WRAP border (common.h MaterialExtra)
        const uint32_t pw = mw + 2, ph = mh + 2;
        std::vector<uint32_t> texels((size_t)pw * ph);
        const uint8_t *e = static_cast<const uint8_t *>(emissive), *o = static_cast<const uint8_t *>(occlusion);
        for (uint32_t Y = 0; Y < ph; ++Y) {
            const size_t sy = (size_t)((Y + mh - 1) % mh) * mw;
            for (uint32_t X = 0; X < pw; ++X) {
                const size_t i = sy + (X + mw - 1) % mw;
                const uint32_t rgb = e ? ((uint32_t)e[4 * i] | ((uint32_t)e[4 * i + 1] << 8) | ((uint32_t)e[4 * i + 2] << 16)) : 0xFFFFFFu;
                texels[(size_t)Y * pw + X] = rgb | ((o ? (uint32_t)o[4 * i] : 255u) << 24);
            }
        }
        ok = upload(nx.d_fast, texels.data(), texels.size() * 4);
    } else {
        if (emissive) ok = upload(nx.d_emissive, emissive, (size_t)ew * eh * 4);
        if (ok && occlusion) ok = upload(nx.d_occlusion, occlusion, (size_t)ow * oh * 4);
    }
    if (!ok) return r->fail(ARCTIC_E_DEVICE, "set_material_extras: hipMalloc / upload of an image");
    HIPCHECK(r, hipStreamSynchronize(r->stream));   // (a pass in flight may still read the table and the images it replaces)
    ArcticRenderer::Extras &cur = r->extras[material];
    const bool table_changes = !(cur.neutral && nx.neutral);
    r->n_extras += (nx.neutral ? 0u : 1u) - (cur.neutral ? 0u : 1u);
    cur = std::move(nx);   // (the images it replaces go with the assignment)
    return table_changes ? upload_tex_table(r) : ARCTIC_OK;
}

int arctic_create_mesh(ArcticRenderer *r, const ArcticVertex *vertices, uint64_t n_vertices, const uint32_t *indices,
                       uint64_t n_indices, uint64_t material_idx) {
    if (!r) return ARCTIC_E_INVALID;
    if (!vertices || !indices || n_vertices == 0 || n_indices == 0) return r->fail(ARCTIC_E_INVALID, "create_mesh: empty mesh");
    if (n_indices % 3 != 0) return r->fail(ARCTIC_E_INVALID, "create_mesh: index count %llu is not a multiple of 3 (triangle list)", (unsigned long long)n_indices);
    if (material_idx >= r->tex.size() / 3) return r->fail(ARCTIC_E_INVALID, "create_mesh: material %llu does not exist", (unsigned long long)material_idx);
    if (n_vertices > 0x7FFFFFFFull || n_indices > 0xFFFFFFF0ull) return r->fail(ARCTIC_E_CAPACITY, "create_mesh: mesh too large");
    int rc = select_device(r);
    if (rc) return rc;
    Mesh fresh;
    HIPCHECK(r, fresh.d_vertices.alloc_exact(n_vertices * sizeof(ArcticVertex)));
    if (fresh.d_indices.alloc_exact(n_indices * 4) != hipSuccess) return r->fail(ARCTIC_E_DEVICE, "create_mesh: hipMalloc indices");
    fresh.n_vertices = (uint32_t)n_vertices; fresh.n_indices = (uint32_t)n_indices; fresh.material = material_idx;
    cluster_bounds(vertices, fresh.n_vertices, indices, fresh.n_indices, fresh.tbounds, fresh.vbounds);
    r->meshes.push_back(std::move(fresh));
    const Mesh &m = r->meshes.back();
    HIPCHECK(r, hipMemcpy(m.d_vertices.p, vertices, n_vertices * sizeof(ArcticVertex), hipMemcpyHostToDevice));
    HIPCHECK(r, hipMemcpy(m.d_indices.p, indices, n_indices * 4, hipMemcpyHostToDevice));
    return (int)r->meshes.size() - 1;
}

int arctic_check_mesh_skin(const ArcticSkinVertex *skin, uint64_t n_vertices, uint32_t n_joints) {
    return mesh_skin_valid(skin, n_vertices, n_joints) ? ARCTIC_OK : ARCTIC_E_INVALID;
}

int arctic_skin_vertices(const ArcticVertex *in, const ArcticSkinVertex *skin, uint64_t n_vertices, const float *joint_matrices, uint32_t n_joints,
                         ArcticVertex *out) {
    if (!in || !out || !joint_matrices || !mesh_skin_valid(skin, n_vertices, n_joints) || !floats_finite(joint_matrices, (uint64_t)n_joints * 16))
        return ARCTIC_E_INVALID;
    skin_vertices_host(reinterpret_cast<const float *>(in), skin, n_vertices, joint_matrices, reinterpret_cast<float *>(out));
    return ARCTIC_OK;
}

int arctic_set_mesh_skin(ArcticRenderer *r, uint64_t mesh, const ArcticSkinVertex *skin, uint64_t n_vertices, uint32_t n_joints) {
    if (!r) return ARCTIC_E_INVALID;
    if (mesh >= r->meshes.size()) return r->fail(ARCTIC_E_INVALID, "set_mesh_skin: mesh %llu does not exist", (unsigned long long)mesh);
    Mesh &m = r->meshes[mesh];
    DevBuf d_new;
    int rc = select_device(r);
    if (rc) return rc;
    if (skin) {
        if (n_vertices != m.n_vertices) return r->fail(ARCTIC_E_INVALID, "set_mesh_skin: %llu skin records for a mesh of %u vertices", (unsigned long long)n_vertices, m.n_vertices);
        if (!mesh_skin_valid(skin, n_vertices, n_joints))
            return r->fail(ARCTIC_E_INVALID, "set_mesh_skin: n_joints %u outside 1..65535, a joint index at or above it, or a weight that is not finite", n_joints);
        HIPCHECK(r, d_new.alloc_exact(n_vertices * sizeof(ArcticSkinVertex)));
        if (hipMemcpy(d_new.p, skin, n_vertices * sizeof(ArcticSkinVertex), hipMemcpyHostToDevice) != hipSuccess) return r->fail(ARCTIC_E_DEVICE, "set_mesh_skin: upload");
    }
    // what is replaced may still be read: by a k_skin, or -- the posed buffer -- by a prepass; every prepass stream has been joined into the main stream
    if (m.d_skin) HIPCHECK(r, hipStreamSynchronize(r->stream));
    m.release_skin();
    m.d_skin = std::move(d_new); m.n_joints = skin ? n_joints : 0;
    ++m.shape_seq;
    return ARCTIC_OK;
}

int arctic_set_mesh_pose(ArcticRenderer *r, uint64_t mesh, const float *joint_matrices, uint32_t n_joints) {
    if (!r) return ARCTIC_E_INVALID;
    if (mesh >= r->meshes.size()) return r->fail(ARCTIC_E_INVALID, "set_mesh_pose: mesh %llu does not exist", (unsigned long long)mesh);
    Mesh &m = r->meshes[mesh];
    if (!m.d_skin) return r->fail(ARCTIC_E_STATE, "set_mesh_pose: mesh %llu has no skin (arctic_set_mesh_skin)", (unsigned long long)mesh);
    if (!joint_matrices && n_joints == 0) {   // back to the bind pose: the original buffer and the real cluster boxes (the posed buffer is kept for the next pose)
        m.posed = false;
        ++m.shape_seq;
        return ARCTIC_OK;
    }
    if (!joint_matrices || n_joints != m.n_joints) return r->fail(ARCTIC_E_INVALID, "set_mesh_pose: %u joint matrices for a skin of %u joints", n_joints, m.n_joints);
    if (!floats_finite(joint_matrices, (uint64_t)n_joints * 16)) return r->fail(ARCTIC_E_INVALID, "set_mesh_pose: a matrix element is not finite");
    int rc = select_device(r);
    if (rc) return rc;
    const size_t bytes = (size_t)n_joints * 64;
    if (!m.d_posed) HIPCHECK(r, m.d_posed.alloc_exact((size_t)m.n_vertices * sizeof(ArcticVertex)));
    if (!m.d_joints) HIPCHECK(r, m.d_joints.alloc_exact(bytes));
    float *h_joints = nullptr;
    HIPCHECK(r, m.joints_ring.stage(bytes, &h_joints));   // (waits for the copy of POSE_RING poses ago at most)
    std::memcpy(h_joints, joint_matrices, bytes);
    // on the main stream: behind every prepass enqueued so far (arctic_render_frame joins its prepass streams into it), so behind every k_vertex
    // that reads the buffer k_skin overwrites
    HIPCHECK(r, m.joints_ring.send(m.d_joints.p, bytes, r->stream));
    HIPCHECK(r, launch_skin(m.skin_input(), m.d_skin.p, m.d_joints.as<float>(), m.n_vertices, n_joints, m.d_posed.as<float>(), r->stream));
    HIPCHECK(r, r->deformed.record(r->stream));
    m.posed = true;
    ++m.shape_seq;
    return ARCTIC_OK;
}

int arctic_check_morph_targets(const ArcticMorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets) {
    return morph_targets_valid(reinterpret_cast<const float *>(deltas), n_vertices, n_targets) ? ARCTIC_OK : ARCTIC_E_INVALID;
}

int arctic_morph_vertices(const ArcticVertex *in, const ArcticMorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets, const float *weights,
                          ArcticVertex *out) {
    if (!in || !out || !weights || !morph_targets_valid(reinterpret_cast<const float *>(deltas), n_vertices, n_targets) || !floats_finite(weights, n_targets))
        return ARCTIC_E_INVALID;
    morph_vertices_host(reinterpret_cast<const float *>(in), reinterpret_cast<const float *>(deltas), n_vertices, n_targets, weights, reinterpret_cast<float *>(out));
    return ARCTIC_OK;
}

namespace {
// a posed mesh whose k_skin input has just changed (another blend, or none): the pose again, from the matrices the mesh holds
int reskin(ArcticRenderer *r, Mesh &m) {
    if (m.posed) HIPCHECK(r, launch_skin(m.skin_input(), m.d_skin.p, m.d_joints.as<float>(), m.n_vertices, m.n_joints, m.d_posed.as<float>(), r->stream));
    return ARCTIC_OK;
}
// behind the last deformation kernel of a call: what the shadow and prepass streams wait for (wait_skin)
int deformed_on_main_stream(ArcticRenderer *r) {
    HIPCHECK(r, r->deformed.record(r->stream));
    return ARCTIC_OK;
}
}  // namespace

int arctic_set_mesh_morph_targets(ArcticRenderer *r, uint64_t mesh, const ArcticMorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets) {
    if (!r) return ARCTIC_E_INVALID;
    if (mesh >= r->meshes.size()) return r->fail(ARCTIC_E_INVALID, "set_mesh_morph_targets: mesh %llu does not exist", (unsigned long long)mesh);
    Mesh &m = r->meshes[mesh];
    DevBuf d_new;
    int rc = select_device(r);
    if (rc) return rc;
    if (deltas) {
        if (n_vertices != m.n_vertices) return r->fail(ARCTIC_E_INVALID, "set_mesh_morph_targets: %llu records per target for a mesh of %u vertices", (unsigned long long)n_vertices, m.n_vertices);
        if (!morph_targets_valid(reinterpret_cast<const float *>(deltas), n_vertices, n_targets))
            return r->fail(ARCTIC_E_INVALID, "set_mesh_morph_targets: n_targets %u outside 1..65535, or a delta that is not finite", n_targets);
        const size_t bytes = (size_t)n_targets * n_vertices * sizeof(ArcticMorphDelta);
        if (d_new.alloc_exact(bytes) != hipSuccess) {
            (void)hipGetLastError();
            return r->fail(ARCTIC_E_DEVICE, "set_mesh_morph_targets: %u targets x %llu vertices x 48 bytes cannot be allocated", n_targets, (unsigned long long)n_vertices);
        }
        if (hipMemcpy(d_new.p, deltas, bytes, hipMemcpyHostToDevice) != hipSuccess) return r->fail(ARCTIC_E_DEVICE, "set_mesh_morph_targets: upload");
    }
    // what is replaced may still be read: by a k_morph, a k_skin, or -- the blended buffer -- by a prepass; every prepass stream has been joined
    // into the main stream
    const bool was_morphed = m.morphed;
    if (m.d_deltas && hipStreamSynchronize(r->stream) != hipSuccess) return r->fail(ARCTIC_E_DEVICE, "set_mesh_morph_targets: hipStreamSynchronize");
    m.release_morph();
    m.d_deltas = std::move(d_new); m.n_targets = deltas ? n_targets : 0;
    m.morph_weights.assign(m.n_targets, 0.0f);
    ++m.shape_seq;
    if (was_morphed && m.posed) {   // the pose stood on the blend that has just gone: once more, on the mesh's own vertices (the stream is drained)
        if ((rc = reskin(r, m)) != ARCTIC_OK) return rc;
        return deformed_on_main_stream(r);
    }
    return ARCTIC_OK;
}

int arctic_set_mesh_morph_weights(ArcticRenderer *r, uint64_t mesh, const float *weights, uint32_t n_targets) {
    if (!r) return ARCTIC_E_INVALID;
    if (mesh >= r->meshes.size()) return r->fail(ARCTIC_E_INVALID, "set_mesh_morph_weights: mesh %llu does not exist", (unsigned long long)mesh);
    Mesh &m = r->meshes[mesh];
    if (!m.d_deltas) return r->fail(ARCTIC_E_STATE, "set_mesh_morph_weights: mesh %llu has no morph targets (arctic_set_mesh_morph_targets)", (unsigned long long)mesh);
    const bool rest = !weights && n_targets == 0;
    if (!rest) {
        if (!weights || n_targets != m.n_targets) return r->fail(ARCTIC_E_INVALID, "set_mesh_morph_weights: %u weights for a mesh of %u targets", n_targets, m.n_targets);
        if (!floats_finite(weights, n_targets)) return r->fail(ARCTIC_E_INVALID, "set_mesh_morph_weights: a weight is not finite");
    }
    int rc = select_device(r);
    if (rc) return rc;
    // the targets that take part: non-zero weight (either sign of zero is skipped), ascending index
    std::vector<MorphActive> active;
    if (!rest) for (uint32_t k = 0; k < n_targets; ++k) if (weights[k] != 0.0f) active.push_back({k, weights[k]});
    // Everything below is enqueued on the main stream: behind every prepass enqueued so far (arctic_render_frame joins its prepass streams into
    // it), so behind every k_vertex and k_skin that reads the buffers k_morph and k_skin overwrite
    if (active.empty()) {   // the mesh's own vertices again: no blend (the blended buffer is kept for the next call)
        const bool was_morphed = m.morphed;
        m.morphed = false;
        if (was_morphed && m.posed) {
            if ((rc = reskin(r, m)) != ARCTIC_OK || (rc = deformed_on_main_stream(r)) != ARCTIC_OK) { m.morphed = true; return rc; }
        }
    } else {
        const size_t cap = (size_t)m.n_targets * sizeof(MorphActive), bytes = active.size() * sizeof(MorphActive);
        if (!m.d_morphed) HIPCHECK(r, m.d_morphed.alloc_exact((size_t)m.n_vertices * sizeof(ArcticVertex)));
        if (!m.d_active) HIPCHECK(r, m.d_active.alloc_exact(cap));
        MorphActive *h_active = nullptr;
        HIPCHECK(r, m.active_ring.stage(cap, &h_active));   // (waits for the copy of POSE_RING calls ago at most)
        std::memcpy(h_active, active.data(), bytes);
        HIPCHECK(r, m.active_ring.send(m.d_active.p, bytes, r->stream));
        HIPCHECK(r, launch_morph(m.d_vertices.as<float>(), m.d_deltas.as<float>(), m.d_active.as<MorphActive>(), (uint32_t)active.size(), m.n_vertices, m.d_morphed.as<float>(), r->stream));
        m.morphed = true;
        if ((rc = reskin(r, m)) != ARCTIC_OK) return rc;
        if ((rc = deformed_on_main_stream(r)) != ARCTIC_OK) return rc;
    }
    if (rest) m.morph_weights.assign(m.n_targets, 0.0f);
    else m.morph_weights.assign(weights, weights + n_targets);
    ++m.shape_seq;
    return ARCTIC_OK;
}

int arctic_read_mesh_vertices(ArcticRenderer *r, uint64_t mesh, ArcticVertex *out, uint64_t n_vertices) {
    if (!r) return ARCTIC_E_INVALID;
    if (mesh >= r->meshes.size()) return r->fail(ARCTIC_E_INVALID, "read_mesh_vertices: mesh %llu does not exist", (unsigned long long)mesh);
    const Mesh &m = r->meshes[mesh];
    if (!out || n_vertices != m.n_vertices) return r->fail(ARCTIC_E_INVALID, "read_mesh_vertices: room for %llu vertices, the mesh has %u", (unsigned long long)n_vertices, m.n_vertices);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    HIPCHECK(r, hipMemcpy(out, m.vertices_in_use(), n_vertices * sizeof(ArcticVertex), hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

// ---- the pair table of the packed light loop (common.h: ShadeParams::light_pairs, pair_runs; the exactness contract: shade.hip, accumulate_pair) ----
// A light whose colour channel is +0.0f BY ITS BITS adds +-0 to that channel's three sums; a pair of two such lights needs none of the three
// packed multiply-adds.  (-0.0f, denormals, NaN and Inf count as non-zero: only +0 leaves the sums' bits alone whatever it is multiplied with.)
// The table is therefore built from a stable partition of the lights by the lowest zero channel (class 0, 1, 2 = R, G, B; 3 = none), pairs are
// formed along that sequence -- the odd light at the end of a class pairs with the first light of the next, the black partner of an odd total
// (mask 7) comes last -- and the pairs are laid out, stably, as four runs: skip R, skip G, skip B, general.  A pair's mask is the AND of its
// lights' masks; it goes to the run of its lowest set bit, the partner's pair always to the end of the general run (the counting kernels know
// the partner by its place).  runs = false: caller order, one general run -- the table of earlier builds.
namespace {
constexpr uint32_t PAIR_PARTNER = 0xFFFFFFFFu;   // slot of the black partner
uint32_t zero_channels(const ArcticPointLight &l) {
    uint32_t m = 0;
    for (int c = 0; c < 3; ++c) { uint32_t b; std::memcpy(&b, &l.color[c], 4); m |= (b == 0u ? 1u : 0u) << c; }
    return m;
}
uint32_t run_of_mask(uint32_t m) { return m & 1u ? 0u : m & 2u ? 1u : m & 4u ? 2u : 3u; }
// slots: 2 * n_pairs light indices (pair p = slots[2p], slots[2p + 1]); masks: n_pairs; run_end: where the runs R, G and B end (the general run ends at n_pairs)
void light_pair_table(const ArcticPointLight *lights, uint32_t k, bool runs, std::vector<uint32_t> &slots, std::vector<uint32_t> &masks, uint32_t run_end[3]) {
    const uint32_t n_pairs = (k + 1) / 2;
    std::vector<uint32_t> seq; seq.reserve(2 * (size_t)n_pairs);
    if (runs && n_pairs <= PAIR_RUN_MAX) {
        for (uint32_t c = 0; c < 4; ++c)
            for (uint32_t i = 0; i < k; ++i) if (run_of_mask(zero_channels(lights[i])) == c) seq.push_back(i);
    } else {
        runs = false;
        for (uint32_t i = 0; i < k; ++i) seq.push_back(i);
    }
    if (k & 1u) seq.push_back(PAIR_PARTNER);
    auto mask_of = [&](uint32_t s) { return s == PAIR_PARTNER ? 7u : zero_channels(lights[s]); };
    slots.clear(); masks.clear();
    uint32_t end[4] = {0, 0, 0, 0};
    for (uint32_t c = 0; c < 4; ++c) {
        for (uint32_t p = 0; p < n_pairs; ++p) {
            const uint32_t a = seq[2 * p], b = seq[2 * p + 1], m = mask_of(a) & mask_of(b);
            if ((runs && b != PAIR_PARTNER ? run_of_mask(m) : 3u) != c) continue;
            slots.push_back(a); slots.push_back(b); masks.push_back(m);
        }
        end[c] = (uint32_t)masks.size();
    }
    run_end[0] = end[0]; run_end[1] = end[1]; run_end[2] = end[2];
}
}   // namespace

// the table as plain numbers (a pure host function: tests/test_light_pair_table.py)
int arctic_light_pair_table(const ArcticPointLight *lights, uint64_t n, int32_t runs, uint32_t *slots, uint32_t *masks, uint32_t *run_end) {
    if ((n && !lights) || n > 0x7FFFFFFFull || (n && (!slots || !masks)) || !run_end) return ARCTIC_E_INVALID;
    std::vector<uint32_t> s, m;
    light_pair_table(lights, (uint32_t)n, runs != 0, s, m, run_end);
    if (!s.empty()) std::memcpy(slots, s.data(), s.size() * 4);
    if (!m.empty()) std::memcpy(masks, m.data(), m.size() * 4);
    return ARCTIC_OK;
}

namespace {
// the handle's lights as pairs for the packed loop; an odd count gets a black partner
int upload_light_pairs(ArcticRenderer *r) {
    const ArcticPointLight *lights = r->h_lights.data();
    const uint32_t k = (uint32_t)r->h_lights.size(), n_pairs = (k + 1) / 2;
    std::vector<uint32_t> slots, masks;
    uint32_t run_end[3];
    light_pair_table(lights, k, r->light_pair_runs != 0, slots, masks, run_end);
    std::vector<float> pairs((size_t)std::max(1u, n_pairs) * 12, 0.0f);
    for (uint32_t i = 0; i < 2 * n_pairs; ++i) {
        float *dst = pairs.data() + (size_t)(i / 2) * 12 + (i & 1);
        const uint32_t s = slots[i];
        if (s != PAIR_PARTNER) { dst[0] = lights[s].position[0]; dst[2] = lights[s].position[1]; dst[4] = lights[s].position[2];
                                 dst[6] = lights[s].color[0]; dst[8] = lights[s].color[1]; dst[10] = lights[s].color[2]; }
        else { dst[0] = 0.0f; dst[2] = 1.0e6f; dst[4] = 0.0f; dst[6] = dst[8] = dst[10] = 0.0f; }
    }
    HIPCHECK(r, r->d_light_pairs.ensure(pairs.size() * 4));
    HIPCHECK(r, hipMemcpy(r->d_light_pairs.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
    r->pair_runs = run_end[0] | run_end[1] << PAIR_RUN_BITS | run_end[2] << (2 * PAIR_RUN_BITS);
    return ARCTIC_OK;
}
}   // namespace

int arctic_update_lights(ArcticRenderer *r, const ArcticPointLight *lights, uint64_t n) {
    if (!r) return ARCTIC_E_INVALID;
    if (n && !lights) return r->fail(ARCTIC_E_INVALID, "update_lights: null");
    int rc = select_device(r);
    if (rc) return rc;
    uint32_t k = (uint32_t)std::min<uint64_t>(n, r->max_lights);   // renderer.cpp:587-588
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (k) HIPCHECK(r, hipMemcpy(r->d_lights.p, lights, (size_t)k * sizeof(ArcticPointLight), hipMemcpyHostToDevice));   // (caller order: the scalar loop, the statistics)
    r->h_lights.assign(lights, lights + k);
    if ((rc = upload_light_pairs(r)) != ARCTIC_OK) return rc;
    r->n_lights = k;
    return ARCTIC_OK;
}

// arctic_update_spot_lights' validation and derivation (include/arctic_hip.h): binary64, each constant rounded once
int arctic_spot_light_constants(const ArcticSpotLight *lights, uint64_t n, float *out) {
    if (n && (!lights || !out)) return ARCTIC_E_INVALID;
    const float PI_F = (float)M_PI;   // "pi": the fp32 value nearest pi (3.14159274)
    for (uint64_t i = 0; i < n; ++i) {
        const ArcticSpotLight &l = lights[i];
        const float *f = l.position;   // 12 floats, no padding
        for (int k = 0; k < 12; ++k) if (!std::isfinite(f[k])) return ARCTIC_E_INVALID;
        const double dx = l.direction[0], dy = l.direction[1], dz = l.direction[2];
        if (dx == 0.0 && dy == 0.0 && dz == 0.0) return ARCTIC_E_INVALID;
        if (!(l.inner_cone_angle >= 0.0f && l.inner_cone_angle <= l.outer_cone_angle && l.outer_cone_angle > 0.0f && l.outer_cone_angle <= PI_F &&
              l.range >= 0.0f)) return ARCTIC_E_INVALID;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const ArcticSpotLight &l = lights[i];
        const double dx = l.direction[0], dy = l.direction[1], dz = l.direction[2];
        const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
        double scale = 0.0, offset = 1.0;
        if (l.outer_cone_angle != PI_F) {
            const double co = std::cos((double)l.outer_cone_angle), ci = std::cos((double)l.inner_cone_angle);
            scale = 1.0 / std::max(1e-3, ci - co);
            offset = -co * scale;
        }
        const double range = l.range;
        const double ir2 = range > 0.0 ? 1.0 / (range * range) : 0.0;
        float *o = out + 12 * i;
        o[0] = l.position[0]; o[1] = l.position[1]; o[2] = l.position[2]; o[3] = (float)scale;
        o[4] = (float)(dx / len); o[5] = (float)(dy / len); o[6] = (float)(dz / len); o[7] = (float)offset;
        o[8] = l.color[0]; o[9] = l.color[1]; o[10] = l.color[2]; o[11] = (float)ir2;
    }
    return ARCTIC_OK;
}

int arctic_update_spot_lights(ArcticRenderer *r, const ArcticSpotLight *lights, uint64_t n) {
    if (!r) return ARCTIC_E_INVALID;
    if (n && !lights) return r->fail(ARCTIC_E_INVALID, "update_spot_lights: null");
    std::vector<float> dev((size_t)std::min<uint64_t>(n, r->max_lights) * 12);
    // (every light given is checked, also those beyond the cap; on failure the handle's list stays as it was)
    float one[12];
    for (uint64_t i = 0; i < n; ++i)
        if (arctic_spot_light_constants(lights + i, 1, one) != ARCTIC_OK)
            return r->fail(ARCTIC_E_INVALID, "update_spot_lights: light %llu: a NaN or inf field, a zero direction, inner > outer, outer outside (0, pi] or range < 0", (unsigned long long)i);
    const uint32_t k = (uint32_t)std::min<uint64_t>(n, r->max_lights);
    int rc = select_device(r);
    if (rc) return rc;
    if (k) {
        (void)arctic_spot_light_constants(lights, k, dev.data());
        HIPCHECK(r, hipStreamSynchronize(r->stream));   // (a pass in flight may still read the list it replaces)
        HIPCHECK(r, r->d_spots.ensure((size_t)k * sizeof(SpotDev)));
        HIPCHECK(r, hipMemcpy(r->d_spots.p, dev.data(), (size_t)k * sizeof(SpotDev), hipMemcpyHostToDevice));
    }
    r->n_spots = k;
    return ARCTIC_OK;
}

// ---- shadow-casting point lights (include/arctic_hip.h) ----------------------------------------------------------------
namespace {
bool valid_cube_light(const ArcticPointShadowLight &l) {
    const float *f = l.position;   // 8 floats, no padding
    for (int k = 0; k < 8; ++k) if (!std::isfinite(f[k])) return false;
    return l.z_near > 0.0f && l.z_near < l.z_far;
}
// room for k lights with faces of F^2 texels; the faces cleared to 1.0 and the records (binary64, each rounded once) uploaded.  A failed
// allocation leaves the handle's buffer and list as they were.  The caller has synchronised the stream.
int cube_store(ArcticRenderer *r, const ArcticPointShadowLight *lights, uint32_t k, uint32_t F) {
    const size_t rec_bytes = (size_t)k * sizeof(CubeDev), bytes = rec_bytes + (size_t)k * 6 * F * F * 4;
    if (bytes > r->d_cubes.cap) {
        DevBuf fresh;
        if (fresh.alloc_exact(bytes) != hipSuccess) { (void)hipGetLastError(); return r->fail(ARCTIC_E_DEVICE, "point shadows: cannot allocate %zu bytes of faces", bytes); }
        r->d_cubes = std::move(fresh);
    }
    if ((size_t)k * 6 > r->cube_count_faces) {   // pinned, mapped counts: 8 words per face
        PinnedBuf fresh;
        const size_t n = (size_t)std::max<uint32_t>(k, r->max_lights) * 6;
        if (fresh.alloc(n * CUBE_COUNT_WORDS * 4, hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            return r->fail(ARCTIC_E_DEVICE, "point shadows: cannot allocate the pinned counters");
        }
        std::memset(fresh.p, 0, n * CUBE_COUNT_WORDS * 4);
        r->cube_counts = std::move(fresh); r->cube_count_faces = (uint32_t)n;
    }
    std::vector<CubeDev> dev(k);
    for (uint32_t i = 0; i < k; ++i) {
        const ArcticPointShadowLight &l = lights[i];
        CubeDev &d = dev[i];
        for (int c = 0; c < 3; ++c) { d.p[c] = l.position[c]; d.c[c] = l.color[c]; }
        d.pz_scale = (float)((double)l.z_far / ((double)l.z_far - (double)l.z_near));
        d.zn = l.z_near;
    }
    HIPCHECK(r, hipMemcpy(r->d_cubes.p, dev.data(), rec_bytes, hipMemcpyHostToDevice));
    HIPCHECK(r, launch_fill_u64(reinterpret_cast<unsigned long long *>(r->d_cubes.as<char>() + rec_bytes), 0x3F8000003F800000ull, (size_t)k * 3 * F * F, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    return ARCTIC_OK;
}
}  // namespace

int arctic_point_shadow_matrices(const ArcticPointShadowLight *light, float *out96) {
    if (!light || !out96 || !valid_cube_light(*light)) return ARCTIC_E_INVALID;
    for (int k = 0; k < 6; ++k) point_shadow_proj_view(light->position, k, light->z_near, light->z_far, out96 + 16 * k);
    return ARCTIC_OK;
}

int arctic_update_point_shadow_lights(ArcticRenderer *r, const ArcticPointShadowLight *lights, uint64_t n) {
    if (!r) return ARCTIC_E_INVALID;
    if (n && !lights) return r->fail(ARCTIC_E_INVALID, "update_point_shadow_lights: null");
    // (every light given is checked, also those beyond the cap; on failure the handle's list and faces stay as they were)
    for (uint64_t i = 0; i < n; ++i)
        if (!valid_cube_light(lights[i]))
            return r->fail(ARCTIC_E_INVALID, "update_point_shadow_lights: light %llu: a NaN or inf field, z_near <= 0 or z_far <= z_near", (unsigned long long)i);
    const uint32_t k = (uint32_t)std::min<uint64_t>(n, r->max_lights);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));   // (a pass in flight may still read the faces it replaces)
    if (k) {
        r->n_cubes = 0;   // (cube_store's layout: records of the new list first)
        rc = cube_store(r, lights, k, r->cube_size);
        if (rc != ARCTIC_OK) {   // the previous records and faces are untouched unless the buffer was reused: put the old list back
            if (!r->cube_lights.empty()) r->n_cubes = (uint32_t)r->cube_lights.size();
            return rc;
        }
    }
    r->cube_lights.assign(lights, lights + k);
    r->n_cubes = k;
    r->cube_key.clear();
    r->cube_faces_filled = false;   // (cleared to 1.0: nothing has been drawn into them)
    return ARCTIC_OK;
}

int arctic_pass_point_shadows(ArcticRenderer *r, const ArcticScene *scene) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "pass_point_shadows: bad scene");
    int rc = select_device(r);
    if (rc) return rc;
    r->cube_key.clear();   // an explicit pass always draws; render_frame's cache starts over
    return pass_point_shadows(r, scene, r->stream);
}

int arctic_read_point_shadow(ArcticRenderer *r, uint32_t light, float *faces) {
    if (!r) return ARCTIC_E_INVALID;
    if (!faces || light >= r->n_cubes) return r->fail(ARCTIC_E_INVALID, "read_point_shadow: null, or light %u of %u", light, r->n_cubes);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    const size_t n = (size_t)6 * r->cube_size * r->cube_size;
    HIPCHECK(r, hipMemcpy(faces, cube_faces(r) + light * n, n * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_write_point_shadow(ArcticRenderer *r, uint32_t light, const float *faces) {
    if (!r) return ARCTIC_E_INVALID;
    if (!faces || light >= r->n_cubes) return r->fail(ARCTIC_E_INVALID, "write_point_shadow: null, or light %u of %u", light, r->n_cubes);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t n = (size_t)6 * r->cube_size * r->cube_size;
    HIPCHECK(r, hipMemcpy(cube_faces(r) + light * n, faces, n * 4, hipMemcpyHostToDevice));
    r->cube_key.clear();
    r->cube_faces_filled = true;
    return ARCTIC_OK;
}

int arctic_create_hdri(ArcticRenderer *r, const float *rgba32f, uint32_t w, uint32_t h) {
    if (!r) return ARCTIC_E_INVALID;
    if (!rgba32f || !w || !h) return r->fail(ARCTIC_E_INVALID, "create_hdri: null image or zero size");
    if ((w | h) & 0xFFFF0000u) return r->fail(ARCTIC_E_CAPACITY, "create_hdri: image side above 65535");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    HIPCHECK(r, r->d_env.ensure((size_t)w * h * 16));
    HIPCHECK(r, hipMemcpy(r->d_env.p, rgba32f, (size_t)w * h * 16, hipMemcpyHostToDevice));
    r->env_w = w; r->env_h = h;
    r->env_built = false;   // a new map: new tables (now, or when the option is set)
    return r->env_lighting == 1 ? build_env_tables(r) : ARCTIC_OK;
}

int arctic_pass_shadow_map(ArcticRenderer *r, const ArcticScene *scene) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "pass_shadow_map: bad scene");
    int rc = select_device(r);
    if (rc) return rc;
    r->shadow_key.clear();   // an explicit pass always renders; render_frame's cache starts over
    return pass_shadow_map(r, scene, r->stream);
}

int arctic_pass_gbuffer(ArcticRenderer *r, const ArcticScene *scene) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "pass_gbuffer: bad scene");
    int rc = select_device(r);
    return rc ? rc : pass_gbuffer(r, scene);
}

int arctic_pass_shade(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, void *d_out) {
    if (!r) return ARCTIC_E_INVALID;
    if (!scene || !settings) return r->fail(ARCTIC_E_INVALID, "pass_shade: null scene/settings");
    int rc = select_device(r);
    return rc ? rc : pass_shade(r, scene, settings, d_out);
}

int arctic_render_frame_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, void *d_out) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene) || !settings) return r->fail(ARCTIC_E_INVALID, "render_frame: bad scene/settings");
    int rc = select_device(r);
    if (rc) return rc;
    std::vector<uint8_t> key = shadow_inputs(r, scene);
    // The shadow pass and the visibility prepass of a frame are independent until the shading pass, and both are bound by latency
    // and by the memory side's atomic rate, not by the ALUs: when the map has to be redrawn it is drawn on
    // a second stream, forked after everything enqueued so far (the previous frame still reads the map) and joined before the
    // shading pass.  (Not with a sharded map: its all-gather stays on the main stream.  ARCTIC_OPT_DEBUG bit 7: one after the other.)
    const bool redraw = r->shadow_size != 0 && (!r->shadow_cache || key != r->shadow_key);
    const bool beside = redraw && !(r->debug & 128) && !(r->shadow_sharded && r->comm && r->comm_world > 1);
    // ... and with frames in flight into the OTHER shadow map, ordered only after what had been enqueued when that one was last
    // left: the pass then runs beside the previous frame's shading too
    const bool shadow_in_flight = beside && r->frames_in_flight > 1;
    if (redraw) {
        r->shadow_key.clear();
        if (beside) {
            if (shadow_in_flight) {
                HIPCHECK(r, r->shadow_set_released[r->scur].record(r->stream));
                r->scur ^= 1;
                HIPCHECK(r, r->d_shadow().ensure(shadow_alloc_bytes(r)));   // first use of the second map (cleared by the pass itself)
                HIPCHECK(r, r->shadow_set_released[r->scur].wait(r->shadow_stream));
            } else {
                HIPCHECK(r, r->shadow_fork.record(r->stream));
                HIPCHECK(r, r->shadow_fork.wait(r->shadow_stream));
            }
            rc = wait_skin(r, r->shadow_stream, r->skin_seen_shadow);
            if (rc == ARCTIC_OK) rc = pass_shadow_map(r, scene, r->shadow_stream);
            if (rc == ARCTIC_OK && !(r->debug & 8)) rc = build_shadow_bounds(r, r->shadow_stream);
            HIPCHECK(r, r->shadow_drawn.record(r->shadow_stream));
        } else rc = pass_shadow_map(r, scene, r->stream);
        if (rc != ARCTIC_OK) { if (beside) (void)r->shadow_drawn.wait(r->stream); return rc; }
        r->shadow_key.swap(key);
    }
    // whole frames skip the G-buffer: the shading pass interpolates from the visibility plane (k_material_vis), bit-identical
    // to visibility -> G-buffer -> shading; arctic_read_gbuffer / arctic_pass_shade materialise the G-buffer afterwards if asked
    const bool vis_path = r->visbuffer;
    // frames in flight: this frame's visibility prepass goes to the other table set, on prepass_stream, ordered only after what
    // the main stream had enqueued when that set was last left -- so it runs beside the shading of the previous frame
    // (not in a frame that redraws the shadow map on the main stream -- sharded map, debug bit 7 --: that pass has to follow the previous
    // frame's shading and precede this one's, a prepass running ahead would only compete with it)
    const bool in_flight = vis_path && r->frames_in_flight > 1 && (!redraw || shadow_in_flight);
    if (in_flight) {
        HIPCHECK(r, r->vis_set_released[r->cur].record(r->stream));   // everything that reads or writes the set being left is enqueued by now
        r->cur = (r->cur + 1) % r->frames_in_flight;
        r->have_vis = r->have_gbuffer = r->have_order = false;            // of the set entered: overwritten now
        // consecutive prepasses on alternate streams when there are three sets (they overlap then); with two, one stream as before
        const int turn = r->frames_in_flight >= 3 ? (r->prepass_turn ^= 1) : 0;
        hipStream_t ps = r->prepass_stream[0];
        if (turn) {
            if (r->own_stream_is_prepass()) ps = r->own_stream;
            else { if (!r->prepass_stream[1]) HIPCHECK(r, r->prepass_stream[1].create(hipStreamNonBlocking)); ps = r->prepass_stream[1]; }
        }
        HIPCHECK(r, r->vis_set_released[r->cur].wait(ps));
        rc = wait_skin(r, ps, r->skin_seen_prepass[turn]);
        if (rc == ARCTIC_OK) rc = pass_visibility(r, scene, ps);
        HIPCHECK(r, r->prepass_done[turn].record(ps));
        HIPCHECK(r, r->prepass_done[turn].wait(r->stream));
    } else rc = vis_path ? pass_visibility(r, scene, r->stream) : pass_gbuffer(r, scene);
    if (beside) HIPCHECK(r, r->shadow_drawn.wait(r->stream));   // the map and its table are complete
    if (rc != ARCTIC_OK) return rc;
    // the point lights' faces: redrawn when their inputs changed, on the main stream -- behind the previous frame's shading, which reads
    // the one set of faces, and in front of this frame's
    if (r->n_cubes) {
        std::vector<uint8_t> ckey = cube_inputs(r, scene);
        if (!r->shadow_cache || ckey != r->cube_key) {
            r->cube_key.clear();
            rc = pass_point_shadows(r, scene, r->stream);
            if (rc != ARCTIC_OK) return rc;
            r->cube_key.swap(ckey);
        }
    }
    return pass_shade(r, scene, settings, d_out, vis_path);
}

int arctic_render_frame(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, uint8_t *out_rgba8) {
    int rc = arctic_render_frame_device(r, scene, settings, nullptr);
    if (rc != ARCTIC_OK) return rc;
    if (out_rgba8) HIPCHECK(r, hipMemcpyAsync(out_rgba8, r->rgba8_output(), (size_t)r->rows() * r->width * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    return ARCTIC_OK;
}

int arctic_post_process(ArcticRenderer *r, const float *hdr, uint32_t w, uint32_t h, const ArcticSettings *st, uint8_t *out_rgba8,
                        float *out_ldr) {
    if (!r) return ARCTIC_E_INVALID;
    if (!hdr || !w || !h || !st || !out_rgba8) return r->fail(ARCTIC_E_INVALID, "post_process: null argument or zero size");
    int rc = select_device(r);
    if (rc) return rc;
    size_t n = (size_t)w * h;
    HIPCHECK(r, r->d_stage.ensure(n * 16 + n * 4 + n * 12));
    char *base = r->d_stage.as<char>();
    float4 *d_in = reinterpret_cast<float4 *>(base);
    uint8_t *d_out = reinterpret_cast<uint8_t *>(base + n * 16);
    float *d_ldr = reinterpret_cast<float *>(base + n * 20);
    HIPCHECK(r, hipMemcpyAsync(d_in, hdr, n * 16, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, launch_post_process(d_in, w, h, st->tm_method, 1.0f / st->gamma, st->exposure, d_out, out_ldr ? d_ldr : nullptr, r->stream));
    HIPCHECK(r, hipMemcpyAsync(out_rgba8, d_out, n * 4, hipMemcpyDeviceToHost, r->stream));
    if (out_ldr) HIPCHECK(r, hipMemcpyAsync(out_ldr, d_ldr, n * 12, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    return ARCTIC_OK;
}

int arctic_time_shade(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, uint32_t warmup, uint32_t iters,
                      float *ms_each) {
    if (!r) return ARCTIC_E_INVALID;
    if (!scene || !settings || !ms_each || iters == 0) return r->fail(ARCTIC_E_INVALID, "time_shade: bad arguments");
    int rc = select_device(r);
    if (rc) return rc;
    ShadeParams sp;
    if ((rc = fill_shade_params(r, scene, settings, nullptr, sp)) != ARCTIC_OK) return rc;
    for (uint32_t i = 0; i < warmup; ++i) HIPCHECK(r, shade_once(r, sp, false, false));
    std::vector<Event> ev(2 * (size_t)iters);
    for (auto &e : ev) HIPCHECK(r, e.create(hipEventDefault));
    for (uint32_t i = 0; i < iters; ++i) {
        HIPCHECK(r, hipEventRecord(ev[2 * i], r->stream));
        HIPCHECK(r, shade_once(r, sp, false, false));
        HIPCHECK(r, hipEventRecord(ev[2 * i + 1], r->stream));
    }
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    for (uint32_t i = 0; i < iters; ++i) HIPCHECK(r, hipEventElapsedTime(&ms_each[i], ev[2 * i], ev[2 * i + 1]));
    r->have_output = true;
    r->hdr_valid = r->keep_float != 0;
    r->output_filtered = false;   // (the shading kernel alone: d_rgba8 holds what it wrote)
    return ARCTIC_OK;
}

int arctic_antialias_device(ArcticRenderer *r, const void *d_in, void *d_out, uint32_t width, uint32_t height) {
    if (!r) return ARCTIC_E_INVALID;
    if (!d_in || !d_out || !width || !height) return r->fail(ARCTIC_E_INVALID, "antialias: null pointer or zero size");
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    const uint64_t bytes = (uint64_t)width * height * 4;
    if ((a | b) & 3) return r->fail(ARCTIC_E_INVALID, "antialias: RGBA8 images are 4-byte aligned");
    if (a < b + bytes && b < a + bytes) return r->fail(ARCTIC_E_INVALID, "antialias: the input and the output overlap (the filter reads neighbours: not in place)");
    int rc = select_device(r);
    if (rc) return rc;
    Range zone("Anti-aliasing Pass");
    HIPCHECK(r, launch_antialias(d_in, d_out, width, height, r->stream));
    return ARCTIC_OK;
}

int arctic_antialias(ArcticRenderer *r, const uint8_t *rgba8, uint32_t width, uint32_t height, uint8_t *out) {
    if (!r) return ARCTIC_E_INVALID;
    if (!rgba8 || !out || !width || !height) return r->fail(ARCTIC_E_INVALID, "antialias: null pointer or zero size");
    int rc = select_device(r);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 4, half = (n + 255) & ~(size_t)255;
    HIPCHECK(r, hipStreamSynchronize(r->stream));   // (d_stage may move)
    HIPCHECK(r, r->d_stage.ensure(2 * half));
    char *d_in = r->d_stage.as<char>(), *d_out = d_in + half;
    HIPCHECK(r, hipMemcpyAsync(d_in, rgba8, n, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, launch_antialias(d_in, d_out, width, height, r->stream));
    HIPCHECK(r, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    return ARCTIC_OK;
}

int arctic_read_gbuffer(ArcticRenderer *r, float *attrs, uint32_t *material, float *depth, uint32_t *tri) {
    if (!r) return ARCTIC_E_INVALID;
    if (!r->have_gbuffer) {
        if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "read_gbuffer: no G-buffer");
        int rs = select_device(r);
        if (rs) return rs;
        if ((rs = resolve_gbuffer(r)) != ARCTIC_OK) return rs;   // the frame was shaded from the visibility plane
    }
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    size_t px = (size_t)r->rows() * r->width;
    if (attrs || material) {
        HIPCHECK(r, r->d_stage.ensure(px * 76));
        float *d_attrs = r->d_stage.as<float>();
        uint32_t *d_mat = reinterpret_cast<uint32_t *>(r->d_stage.as<char>() + px * 72);
        HIPCHECK(r, launch_gbuffer_tile(r->gbuffer(), d_attrs, d_mat, r->width, r->rows(), r->row0_in_tile, r->tiles_x, r->tiles_y, 0, r->stream));
        if (attrs) HIPCHECK(r, hipMemcpyAsync(attrs, d_attrs, px * 72, hipMemcpyDeviceToHost, r->stream));
        if (material) HIPCHECK(r, hipMemcpyAsync(material, d_mat, px * 4, hipMemcpyDeviceToHost, r->stream));
        HIPCHECK(r, hipStreamSynchronize(r->stream));
    }
    if (depth || tri) {
        // both come straight from the visibility plane the prepass resolved: key = depth bits << 32 | order id, and
        // order id = 8 * (draw-order index of the source triangle) + sub-triangle (k_setup); ~0 = nothing drawn
        if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "read_gbuffer: depth / triangle ids exist only after arctic_pass_gbuffer (not after arctic_write_gbuffer)");
        size_t tp = r->n_tiles() * TILE_PIXELS;
        std::vector<unsigned long long> hv(tp);
        HIPCHECK(r, hipStreamSynchronize(r->stream));
        HIPCHECK(r, hipMemcpy(hv.data(), r->d_vis().p, tp * 8, hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < r->rows(); ++y)
            for (uint32_t x = 0; x < r->width; ++x) {
                uint32_t yy = y + r->row0_in_tile;
                size_t idx = ((size_t)(yy / 8) * r->tiles_x + x / 8) * 64 + (yy % 8) * 8 + (x % 8);
                const unsigned long long key = hv[idx];
                const uint32_t zb = key == ~0ull ? 0x3F800000u : (uint32_t)(key >> 32);
                if (depth) std::memcpy(&depth[(size_t)y * r->width + x], &zb, 4);
                if (tri) tri[(size_t)y * r->width + x] = key == ~0ull ? 0xFFFFFFFFu : (uint32_t)key >> 3;
            }
    }
    return ARCTIC_OK;
}

int arctic_write_gbuffer(ArcticRenderer *r, const float *attrs, const uint32_t *material) {
    if (!r) return ARCTIC_E_INVALID;
    if (!attrs || !material) return r->fail(ARCTIC_E_INVALID, "write_gbuffer: null");
    int rc = select_device(r);
    if (rc) return rc;
    size_t px = (size_t)r->rows() * r->width;
    HIPCHECK(r, r->d_stage.ensure(px * 76));
    float *d_attrs = r->d_stage.as<float>();
    uint32_t *d_mat = reinterpret_cast<uint32_t *>(r->d_stage.as<char>() + px * 72);
    HIPCHECK(r, hipMemcpyAsync(d_attrs, attrs, px * 72, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, hipMemcpyAsync(d_mat, material, px * 4, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, launch_gbuffer_tile(r->gbuffer(), d_attrs, d_mat, r->width, r->rows(), r->row0_in_tile, r->tiles_x, r->tiles_y, 1, r->stream));
    r->lod_valid = false;
    if (r->texture_mips) {   // an injected G-buffer has no triangles: its level-of-detail plane is 0 until arctic_write_lod injects one
        HIPCHECK(r, r->d_lod.ensure(r->n_tiles() * TILE_PIXELS * 4));
        HIPCHECK(r, hipMemsetAsync(r->d_lod.p, 0, r->n_tiles() * TILE_PIXELS * 4, r->stream));
        r->lod_valid = true;
    }
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    r->have_vis = false;
    r->have_gbuffer = true;
    r->have_order = false;   // (a caller's G-buffer comes without cost classes: the geometric order)
    return ARCTIC_OK;
}

int arctic_read_lod(ArcticRenderer *r, float *lod) {
    if (!r) return ARCTIC_E_INVALID;
    if (!lod) return r->fail(ARCTIC_E_INVALID, "read_lod: null");
    if (!r->texture_mips) return r->fail(ARCTIC_E_STATE, "read_lod: no level-of-detail plane (ARCTIC_OPT_TEXTURE_MIPS is 0)");
    int rc = select_device(r);
    if (rc) return rc;
    if (!r->have_gbuffer || !r->lod_valid) {
        if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "read_lod: no G-buffer");
        if ((rc = resolve_gbuffer(r)) != ARCTIC_OK) return rc;   // the frame was shaded from the visibility plane, or resolved with the option off
    }
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    const size_t px = (size_t)r->rows() * r->width;
    HIPCHECK(r, r->d_stage.ensure(px * 4));
    HIPCHECK(r, launch_plane_tile(r->d_lod.as<float>(), r->d_stage.as<float>(), r->width, r->rows(), r->row0_in_tile, r->tiles_x, r->tiles_y, 0, r->stream));
    HIPCHECK(r, hipMemcpyAsync(lod, r->d_stage.p, px * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    return ARCTIC_OK;
}

int arctic_write_lod(ArcticRenderer *r, const float *lod) {
    if (!r) return ARCTIC_E_INVALID;
    if (!lod) return r->fail(ARCTIC_E_INVALID, "write_lod: null");
    if (!r->texture_mips) return r->fail(ARCTIC_E_STATE, "write_lod: no level-of-detail plane (ARCTIC_OPT_TEXTURE_MIPS is 0)");
    if (!r->have_gbuffer) return r->fail(ARCTIC_E_STATE, "write_lod: no G-buffer to go with the plane (arctic_pass_gbuffer or arctic_write_gbuffer first)");
    int rc = select_device(r);
    if (rc) return rc;
    const size_t px = (size_t)r->rows() * r->width;
    HIPCHECK(r, r->d_stage.ensure(px * 4));
    HIPCHECK(r, r->d_lod.ensure(r->n_tiles() * TILE_PIXELS * 4));
    HIPCHECK(r, hipMemcpyAsync(r->d_stage.p, lod, px * 4, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, launch_plane_tile(r->d_lod.as<float>(), r->d_stage.as<float>(), r->width, r->rows(), r->row0_in_tile, r->tiles_x, r->tiles_y, 1, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    r->lod_valid = true;
    return ARCTIC_OK;
}

int arctic_read_material_mip(ArcticRenderer *r, uint32_t material, uint32_t level, uint8_t *texels, uint32_t dims[2]) {
    if (!r) return ARCTIC_E_INVALID;
    if (material >= r->tex.size() / 3) return r->fail(ARCTIC_E_INVALID, "read_material_mip: material %u does not exist", material);
    const TexDesc &d0 = r->tex[3 * (size_t)material];
    if (!(d0.w & TEX_INTERLEAVED)) return r->fail(ARCTIC_E_INVALID, "read_material_mip: material %u has images of unequal sizes (no packed image, one level)", material);
    const std::vector<TexDesc> &chain = r->chains[material];
    const uint32_t levels = chain.empty() ? 1u : (uint32_t)chain.size();
    if (level >= levels) return r->fail(ARCTIC_E_INVALID, "read_material_mip: level %u beyond the material's %u", level, levels);
    const TexDesc &d = chain.empty() ? d0 : chain[level];
    const uint32_t w = d.w & ~TEX_INTERLEAVED, h = d.h;
    if (dims) { dims[0] = w; dims[1] = h; }
    if (!texels) return ARCTIC_OK;   // (the size alone)
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    // the bordered image as stored (row-major or 4 x 4-texel tiles), unpacked on the host: a test's read-back
    const uint32_t pw = w + 2, ph = h + 2, tpr = (pw + 3) / 4, trows = (ph + 3) / 4;
    const size_t bytes = d.tile_row_bytes ? (size_t)tpr * trows * 128 : (size_t)pw * ph * 8;
    std::vector<uint8_t> img(bytes);
    HIPCHECK(r, hipMemcpy(img.data(), d.texels, bytes, hipMemcpyDeviceToHost));
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t X = x + 1, Y = y + 1;
            const size_t o = d.tile_row_bytes ? (size_t)(Y >> 2) * d.tile_row_bytes + (size_t)(X >> 2) * 128 + ((Y & 3) * 4 + (X & 3)) * 8 : ((size_t)Y * pw + X) * 8;
            std::memcpy(texels + ((size_t)y * w + x) * 8, img.data() + o, 8);
        }
    return ARCTIC_OK;
}

int arctic_read_shadow_map(ArcticRenderer *r, float *depth) {
    if (!r) return ARCTIC_E_INVALID;
    if (!depth || !r->shadow_size) return r->fail(ARCTIC_E_INVALID, "read_shadow_map: null or no shadow map");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    HIPCHECK(r, hipMemcpy(depth, r->d_shadow().p, (size_t)r->shadow_size * r->shadow_size * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_write_shadow_map(ArcticRenderer *r, const float *depth) {
    if (!r) return ARCTIC_E_INVALID;
    if (!depth || !r->shadow_size) return r->fail(ARCTIC_E_INVALID, "write_shadow_map: null or no shadow map");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    HIPCHECK(r, hipMemcpy(r->d_shadow().p, depth, (size_t)r->shadow_size * r->shadow_size * 4, hipMemcpyHostToDevice));
    r->shadow_key.clear(); r->bounds_valid() = false;
    r->shadow_written_set[r->scur] = true;
    return ARCTIC_OK;
}

int arctic_read_output(ArcticRenderer *r, float *ldr, float *hdr, uint8_t *rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    if (!r->have_output) return r->fail(ARCTIC_E_STATE, "read_output: nothing shaded into the handle's own buffers yet");
    if ((ldr || hdr) && !r->keep_float) return r->fail(ARCTIC_E_STATE, "read_output: float planes need ARCTIC_OPT_KEEP_FLOAT_OUTPUT");
    int rc = select_device(r);
    if (rc) return rc;
    size_t px = (size_t)r->rows() * r->width;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    if (ldr) HIPCHECK(r, hipMemcpy(ldr, r->d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (hdr) HIPCHECK(r, hipMemcpy(hdr, r->d_hdr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, r->rgba8_output(), px * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_frame_constants(const ArcticScene *scene, float *proj_view, float *light_proj_view, float *sun_dir) {
    if (!scene) return ARCTIC_E_INVALID;
    const ArcticCamera &c = scene->camera;
    if (proj_view) camera_proj_view(c.eye, c.rotation, c.aspect, c.fov_y, c.z_near_far[0], c.z_near_far[1], proj_view);
    if (light_proj_view) sun_proj_view(scene->sun.position, scene->sun.rotation, light_proj_view);
    if (sun_dir) dir_from_rot(scene->sun.rotation, sun_dir);
    return ARCTIC_OK;
}

int arctic_stats(ArcticRenderer *r, uint64_t *out, uint32_t n) {
    if (!r || !out) return ARCTIC_E_INVALID;
    if (select_device(r) == ARCTIC_OK) (void)hipStreamSynchronize(r->stream);
    if (r->h_counts()) for (int i = 0; i < 4; ++i) r->stats[i] = r->h_counts()[i];
    for (uint32_t i = 0; i < n && i < 16; ++i) out[i] = i < 8 ? r->stats[i] : i < 10 ? r->light_stats[i - 8] : i < 12 ? (r->h_counts() ? r->h_counts()[6 + (i - 10)] : 0) : r->edge_stats[i - 12];
    return ARCTIC_OK;
}

// the owner grid as plain numbers (pure host functions: tests/test_owner_grid.py checks that every tile row a shard stores is visited
// exactly once, for layouts no GPU test has time for)
int arctic_owner_grid(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t band_rows, uint32_t shard_index, uint32_t shard_count,
                      uint32_t *grid /* grid_x, grid_y, first block row, 1 = grid rows are the shard's own pairs of tile rows */) {
    if (!grid || !width || !height || (band_rows ? (band_rows % TILE || !shard_count || shard_index >= shard_count) : (row_begin >= row_end || row_end > height))) return ARCTIC_E_INVALID;
    if (band_rows) { row_begin = 0; row_end = height; }
    uint32_t tile_y0, tiles_y;
    shard_tile_rows(height, row_begin, row_end, band_rows, shard_index, band_rows ? shard_count : 1u, tile_y0, tiles_y);
    owner_grid(width, height, tile_y0, tiles_y, band_rows / TILE, grid[0], grid[1], grid[2], grid[3]);
    return ARCTIC_OK;
}
int arctic_owner_visit(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t band_rows, uint32_t shard_index, uint32_t shard_count,
                       uint32_t grid_row, uint32_t *block_row, int32_t *local_tile_rows /* [2]: the shard's tile row stored for the block's upper / lower tile row, -1: none */) {
    uint32_t grid[4];
    const int rc = arctic_owner_grid(width, height, row_begin, row_end, band_rows, shard_index, shard_count, grid);
    if (rc != ARCTIC_OK) return rc;
    if (!block_row || !local_tile_rows || grid_row >= grid[1]) return ARCTIC_E_INVALID;
    if (band_rows) { row_begin = 0; row_end = height; } else shard_count = 1, shard_index = 0;
    uint32_t tile_y0, tiles_y;
    shard_tile_rows(height, row_begin, row_end, band_rows, shard_index, shard_count, tile_y0, tiles_y);
    const int bt = (int)(band_rows / TILE);
    *block_row = owner_block_row(grid_row, grid[2], grid[3], bt, (int)shard_count, (int)shard_index, (int)tile_y0);
    for (int j = 0; j < 2; ++j) {
        int lrow;
        local_tile_rows[j] = owner_tile_row(*block_row, j, (int)tile_y0, (int)tiles_y, bt, (int)shard_count, (int)shard_index, lrow) ? lrow : -1;
    }
    return ARCTIC_OK;
}

// the culling boxes of a mesh as plain numbers (a pure host function: the very cluster_bounds arctic_create_mesh keeps the handle's boxes from;
// tests/test_cluster_bounds.py holds it to its definition and to "a vertex block's box contains its clusters' boxes")
int arctic_cluster_bounds(const ArcticVertex *vertices, uint64_t n_vertices, const uint32_t *indices, uint64_t n_indices, float *tbounds_out, float *vbounds_out) {
    if ((!vertices && n_vertices) || (!indices && n_indices) || n_indices % 3 != 0) return ARCTIC_E_INVALID;
    if (n_vertices > 0x7FFFFFFFull || n_indices > 0xFFFFFFF0ull) return ARCTIC_E_CAPACITY;   // (arctic_create_mesh's limits)
    std::vector<float> tb, vb;
    cluster_bounds(vertices, (uint32_t)n_vertices, indices, (uint32_t)n_indices, tb, vb);
    if ((!tbounds_out && !tb.empty()) || (!vbounds_out && !vb.empty())) return ARCTIC_E_INVALID;
    if (!tb.empty()) std::memcpy(tbounds_out, tb.data(), tb.size() * sizeof(float));
    if (!vb.empty()) std::memcpy(vbounds_out, vb.data(), vb.size() * sizeof(float));
    return ARCTIC_OK;
}

int arctic_read_bin_counts(ArcticRenderer *r, int shadow_pass, uint32_t *out, uint64_t capacity_blocks, uint32_t *blocks_x, uint32_t *blocks_y) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::GeoSet &G = r->geo[shadow_pass ? 1 : r->fwd()];
    if (blocks_x) *blocks_x = G.bins_x;
    if (blocks_y) *blocks_y = G.bins_y;
    const uint64_t n = (uint64_t)G.bins_x * G.bins_y;
    if (!out) return ARCTIC_OK;   // size query
    if (!n) return r->fail(ARCTIC_E_STATE, "read_bin_counts: the latest %s pass had no block owners (ARCTIC_OPT_RASTER_OWNER)", shadow_pass ? "shadow" : "forward");
    if (capacity_blocks < n) return r->fail(ARCTIC_E_CAPACITY, "read_bin_counts: %llu blocks, room for %llu", (unsigned long long)n, (unsigned long long)capacity_blocks);
    int rc = arctic_flush(r);
    if (rc) return rc;
    HIPCHECK(r, hipMemcpy(out, G.d_bin_count.p, n * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_read_cull_counts(ArcticRenderer *r, int shadow_pass, uint32_t *out) {
    if (!r || !out) return ARCTIC_E_INVALID;
    const int set = shadow_pass ? 1 : r->fwd();
    const ArcticRenderer::GeoSet &G = r->geo[set];
    if (!G.cull_counted) return r->fail(ARCTIC_E_STATE, "read_cull_counts: the latest %s pass did not count (ARCTIC_OPT_DEBUG bit 10)", shadow_pass ? "shadow" : "forward");
    int rc = arctic_flush(r);
    if (rc) return rc;
    uint32_t c[N_GEO_COUNTERS];
    HIPCHECK(r, hipMemcpy(c, r->d_geo_counters.as<uint32_t>() + N_GEO_COUNTERS * set, sizeof c, hipMemcpyDeviceToHost));
    out[0] = G.n_tblocks; out[1] = c[5]; out[2] = G.n_vblocks; out[3] = c[6];
    return ARCTIC_OK;
}

int arctic_read_tile_trace(ArcticRenderer *r, uint64_t *out, uint64_t capacity_tiles, uint32_t *tiles_x, uint32_t *tiles_y) {
    if (!r) return ARCTIC_E_INVALID;
    if (tiles_x) *tiles_x = r->tiles_x;
    if (tiles_y) *tiles_y = r->tiles_y;
    const uint64_t n = (uint64_t)r->tiles_x * r->tiles_y;
    if (!out) return ARCTIC_OK;   // size query
    if (!r->tile_trace || r->d_tile_trace.cap < n * 32) return r->fail(ARCTIC_E_STATE, "read_tile_trace: no trace (set ARCTIC_OPT_TILE_TRACE, then shade)");
    if (capacity_tiles < n) return r->fail(ARCTIC_E_CAPACITY, "read_tile_trace: %llu tiles, room for %llu", (unsigned long long)n, (unsigned long long)capacity_tiles);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    HIPCHECK(r, hipMemcpy(out, r->d_tile_trace.p, n * 32, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_read_tile_order(ArcticRenderer *r, uint32_t *order, uint8_t *tile_class, uint64_t capacity_tiles, uint32_t *tiles_x, uint32_t *tiles_y) {
    if (!r) return ARCTIC_E_INVALID;
    if (tiles_x) *tiles_x = r->tiles_x;
    if (tiles_y) *tiles_y = r->tiles_y;
    const uint64_t n = (uint64_t)r->tiles_x * r->tiles_y, n_jobs = (uint64_t)((r->tiles_x + 3) / 4) * r->tiles_y;
    if (!order && !tile_class) return ARCTIC_OK;   // size query
    if (!r->have_order) return r->fail(ARCTIC_E_STATE, "read_tile_order: the G-buffer in place has no dispatch order (ARCTIC_OPT_TILE_ORDER, arctic_pass_gbuffer)");
    if (capacity_tiles < n) return r->fail(ARCTIC_E_CAPACITY, "read_tile_order: %llu tiles, room for %llu", (unsigned long long)n, (unsigned long long)capacity_tiles);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (order) {   // the slots in dispatch order, the empty ones left out: n_jobs entries
        std::vector<uint32_t> slots(r->order_slots);
        HIPCHECK(r, hipMemcpy(slots.data(), r->d_tile_order.p, (size_t)r->order_slots * 4, hipMemcpyDeviceToHost));
        uint64_t k = 0;
        for (uint32_t e : slots) if (e != ORDER_NONE && k < n_jobs) order[k++] = e;
        if (k != n_jobs) return r->fail(ARCTIC_E_STATE, "read_tile_order: %llu strips in the order, %llu in the frame", (unsigned long long)k, (unsigned long long)n_jobs);
    }
    if (tile_class) HIPCHECK(r, hipMemcpy(tile_class, r->d_tile_class.p, n, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_read_env_lighting(ArcticRenderer *r, float *sh27, float *lut, uint32_t level, float *texels, uint32_t *dims) {
    if (!r) return ARCTIC_E_INVALID;
    if (!r->env_built) return r->fail(ARCTIC_E_STATE, "read_env_lighting: no tables (ARCTIC_OPT_ENV_LIGHTING = 1 and an environment map build them)");
    if (level >= ENV_LEVELS) return r->fail(ARCTIC_E_INVALID, "read_env_lighting: level %u of %u", level, ENV_LEVELS);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const EnvTables &T = r->env_host;
    if (dims) { dims[0] = T.w[level]; dims[1] = T.h[level]; dims[2] = ENV_LEVELS; dims[3] = ENV_LUT; }
    if (sh27) HIPCHECK(r, hipMemcpy(sh27, r->d_env_tables.p, 27 * sizeof(float), hipMemcpyDeviceToHost));   // (sh[] is the struct's first member)
    if (lut) HIPCHECK(r, hipMemcpy(lut, T.lut, (size_t)ENV_LUT * ENV_LUT * sizeof(float2), hipMemcpyDeviceToHost));
    if (texels) HIPCHECK(r, hipMemcpy(texels, T.level[level], (size_t)T.w[level] * T.h[level] * sizeof(float4), hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_set_option(ArcticRenderer *r, uint32_t option, int64_t value) {
    if (!r) return ARCTIC_E_INVALID;
    switch (option) {
    case ARCTIC_OPT_KEEP_FLOAT_OUTPUT: r->hdr_valid = r->hdr_valid && r->keep_float && value != 0; r->keep_float = value != 0; break;   // (turned on: the HDR plane is the next shading's)
    case ARCTIC_OPT_COUNT_LIGHT_EVALS: r->count_evals = value != 0; break;
    case ARCTIC_OPT_CULLING: r->culling = value != 0; break;
    case ARCTIC_OPT_DEBUG: r->debug = (int)value; break;
    case ARCTIC_OPT_HDR16: r->hdr16 = value != 0; break;
    case ARCTIC_OPT_VISBUFFER: r->visbuffer = value != 0; break;
    case ARCTIC_OPT_FRAMES_IN_FLIGHT:
        if (value < 0 || value > 3) return r->fail(ARCTIC_E_INVALID, "set_option: frames in flight must be 0 (the library's choice), 1, 2 or 3");
        r->frames_in_flight_opt = (int)value;
        if (value == 0) value = (uint64_t)r->rows() * r->width < 3000000ull ? 3 : 2;
        if ((int)value != r->frames_in_flight) {   // the sets change roles: nothing may be in flight, and `cur` must name a set that exists
            if (int rc = drain_frame_streams(r)) return rc;
            if (r->cur >= (int)value) { r->cur = 0; r->have_vis = r->have_gbuffer = r->have_order = false; }
            for (StreamMark &m : r->vis_set_released) m.forget();
        }
        r->frames_in_flight = (int)value;
        break;
    case ARCTIC_OPT_MARKERS:
        g_markers.enable(value != 0);
        if (value && !g_markers.available()) return r->fail(ARCTIC_E_STATE, "set_option: libroctx64.so could not be loaded");
        break;
    case ARCTIC_OPT_LIGHT_PATH:
        if (value < 0 || value > 2) return r->fail(ARCTIC_E_INVALID, "set_option: light path must be 0..2");
        r->light_path = (int)value;
        break;
    case ARCTIC_OPT_LIGHT_PAIR_RUNS: {
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_LIGHT_PAIR_RUNS: 0 or 1");
        if ((int)value == r->light_pair_runs) break;
        int rc = select_device(r);
        if (rc) return rc;
        HIPCHECK(r, hipStreamSynchronize(r->stream));   // (the table in place may be being read)
        r->light_pair_runs = (int)value;
        if ((rc = upload_light_pairs(r)) != ARCTIC_OK) return rc;
        break;
    }
    case ARCTIC_OPT_ITEM_TABLE_FLOOR:
        if (value < 64 || value > 0x7FFFFFF0ll) return r->fail(ARCTIC_E_INVALID, "set_option: item table floor out of range");
        r->item_cap_floor = (uint32_t)value; r->geo[0].item_cap = r->geo[1].item_cap = r->geo[2].item_cap = r->geo[3].item_cap = 0;
        break;
    case ARCTIC_OPT_TILES_PER_WAVE:
        if (value < 0 || value > 64) return r->fail(ARCTIC_E_INVALID, "set_option: tiles per wave must be 0 (default) .. 64");
        r->tiles_per_wave = (uint32_t)value;
        break;
    case ARCTIC_OPT_TILE_TRACE: r->tile_trace = value != 0; break;
    case ARCTIC_OPT_TEXTURE_TILING: r->texture_tiling = value < 0 ? -1 : (value != 0); break;
    case ARCTIC_OPT_TEXTURE_MIPS:
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_TEXTURE_MIPS: 0 or 1");
        if ((int)value != r->texture_mips) r->lod_valid = false;   // (the plane is made with the next G-buffer, or on demand from the visibility in place)
        r->texture_mips = (int)value;
        break;
    case ARCTIC_OPT_SAMPLER:
        if (value < 0 || (value & ~5ll)) return r->fail(ARCTIC_E_INVALID, "set_option: sampler is a mask of bit 0 (material footprints) and bit 2 (PCF taps); bit 1 (sRGB decode after filtering) exists in the oracle only");
        r->sampler = (int)value;
        break;
    case ARCTIC_OPT_TILE_ORDER: r->tile_order = value != 0; if (!r->tile_order) r->have_order = false; break;
    case ARCTIC_OPT_ORDER_TAIL:
        if (value < 0 || value > 1000) return r->fail(ARCTIC_E_INVALID, "set_option: order tail is per mille, 0..1000");
        r->order_tail = (uint32_t)value;
        break;
    case ARCTIC_OPT_SMALL_TRIANGLES:
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_SMALL_TRIANGLES: 0 or 1");
        r->small_triangles = (int)value; r->shadow_key.clear(); break;
    case ARCTIC_OPT_CLUSTER_CULL:
        if (value < 0 || value > 3 || value == 2) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_CLUSTER_CULL: 0, 1 or 3 (vertex blocks are skipped only where their clusters are)");
        r->cluster_cull = (int)value; r->shadow_key.clear(); break;
    case ARCTIC_OPT_RASTER_OWNER: r->raster_owner = value < 0 ? -1 : (int)(value & 3); r->shadow_key.clear(); break;
    case ARCTIC_OPT_SHADOW_CACHE: r->shadow_cache = value != 0; r->shadow_key.clear(); break;
    case ARCTIC_OPT_SHADOW_SHARDED: r->shadow_sharded = value != 0; r->shadow_key.clear(); break;
    case ARCTIC_OPT_POINT_SHADOW_SIZE: {
        if (value < 8 || value > 4096 || value % 8 != 0) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_POINT_SHADOW_SIZE: a multiple of 8 in [8, 4096]");
        if ((uint32_t)value == r->cube_size) break;
        if (r->n_cubes) {
            int rc = select_device(r);
            if (rc) return rc;
            HIPCHECK(r, hipStreamSynchronize(r->stream));
            rc = cube_store(r, r->cube_lights.data(), r->n_cubes, (uint32_t)value);
            if (rc != ARCTIC_OK) return rc;
        }
        r->cube_size = (uint32_t)value; r->cube_key.clear(); r->cube_faces_filled = false;
        break;
    }
    case ARCTIC_OPT_HIT_MODEL:
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_HIT_MODEL: 0 or 1");
        r->hit_model = (int)value;
        break;
    case ARCTIC_OPT_ANTIALIAS:
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_ANTIALIAS: 0 or 1");
        r->antialias = (int)value;
        break;
    case ARCTIC_OPT_ENV_LIGHTING:
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_ENV_LIGHTING: 0 or 1");
        r->env_lighting = (int)value;
        if (r->env_lighting == 1 && r->env_w && !r->env_built) { int rc = select_device(r); if (rc) return rc; return build_env_tables(r); }
        break;
    case ARCTIC_OPT_RAY_REFIT:
        if (value < 0 || value > 1) return r->fail(ARCTIC_E_INVALID, "ARCTIC_OPT_RAY_REFIT: 0 or 1");
        r->ray.refit_opt = (int)value;   // (in force from the next full build on: a structure built under 0 is not refittable)
        break;
    default: return r->fail(ARCTIC_E_INVALID, "set_option: unknown option %u", option);
    }
    return ARCTIC_OK;
}

}  // extern "C"
