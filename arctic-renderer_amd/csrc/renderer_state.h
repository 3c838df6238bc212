// renderer_state.h -- the handle of the C-ABI, declared once for the host units that implement it: renderer.cpp (create, destroy and resize,
// streams, resources, the passes and frames, options, the debug read-backs), ray_calls.cpp (the ray family, the composition, the motion vectors),
// exchange_calls.cpp (the multi-GPU exchange), one unit per post stage -- taa_calls.cpp, motion_blur_calls.cpp, dof_calls.cpp, bloom_calls.cpp,
// exposure_calls.cpp, fog_calls.cpp, taa_upscale_calls.cpp --, post_source.cpp (what those stages' calls share) and gi_calls.cpp (the indirect diffuse
// light, which runs the ray family's walk and hit shading between kernels of its own).  Also the few helpers one of those units defines and another
// calls.  Host only.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "../../include/arctic_hip.h"
#include "../../include/arctic_dist.h"
#include "common.h"
#include "device_resources.h"

namespace arctic {

// Optional profiler ranges named like the reference's Tracy zones ("Shadow Map Pass", "Forward Pass": shadow_map_pass.cpp:116,
// forward_pass.cpp:164): roctx is loaded at run time only when ARCTIC_OPT_MARKERS is set, so the library has no link-time
// dependency on it.  Host-side ranges around the enqueue of each pass (rocprofv3 --marker-trace shows them).
struct Markers {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false, on = false;
    void enable(bool want) {
        on = want;
        if (want && !tried) {
            tried = true;
            void *h = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
            if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_LOCAL);
            if (h) {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            }
        }
    }
    bool available() const { return push && pop; }
};
extern Markers g_markers;   // (renderer.cpp)
struct Range {
    bool live;
    explicit Range(const char *name) : live(g_markers.on && g_markers.available()) { if (live) g_markers.push(name); }
    ~Range() { if (live) g_markers.pop(); }
};


// RCCL, loaded at run time like roctx (arctic_dist.h): the few entry points the exchange steps use.  Types are declared here
// the way rccl.h declares them (opaque communicator, 128-byte id by value, int enums) so the library needs no RCCL headers.
struct Rccl {
    struct UniqueId { char internal[ARCTIC_COMM_ID_BYTES]; };
    typedef void *Comm;
    static constexpr int Uint8 = 1, Uint32 = 3, Float32 = 7;   // ncclDataType_t (rccl.h:459-466)
    int (*GetUniqueId)(UniqueId *) = nullptr;
    int (*CommInitRank)(Comm *, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(Comm) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, Comm, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, Comm, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, Comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool tried = false;
    bool load() {
        if (!tried) {
            tried = true;
            // an RCCL the process has loaded already (a host that also runs torch.distributed: PyTorch-ROCm brings its own librccl.so.1)
            // is the one to use -- ONE library instance with two communicators, not two RCCL builds side by side on the same devices
            // ARCTIC_RCCL_LIB (honoured only when set): the library that provides the nccl* entry points instead -- the test suite's
            // loopback communicator (tests/cpp/loopback_rccl.cpp: ranks = threads of one process on one GPU, where RCCL refuses two
            // ranks per device), so that the R > 1 branch of the exchange runs where no second GPU exists.  No fallback when it is set.
            const char *override_lib = std::getenv("ARCTIC_RCCL_LIB");
            const bool overridden = override_lib && *override_lib;
            void *h = overridden ? dlopen(override_lib, RTLD_NOW | RTLD_LOCAL) : dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
            if (overridden && !h) return false;
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
            if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
            if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
            if (h) {
                GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
                CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(h, "ncclCommInitRank"));
                CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(h, "ncclCommDestroy"));
                AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(h, "ncclAllGather"));
                Send = reinterpret_cast<decltype(Send)>(dlsym(h, "ncclSend"));
                Recv = reinterpret_cast<decltype(Recv)>(dlsym(h, "ncclRecv"));
                GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(h, "ncclGroupStart"));
                GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(h, "ncclGroupEnd"));
                GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(h, "ncclGetErrorString"));
            }
        }
        return GetUniqueId && CommInitRank && CommDestroy && AllGather && Send && Recv && GroupStart && GroupEnd;
    }
    const char *why(int rc) const { return GetErrorString ? GetErrorString(rc) : "RCCL error"; }
};
extern Rccl g_rccl;   // (exchange_calls.cpp)

// per-pass host->device tables (frame constants, object records, block tables): written into pinned memory and sent with
// ONE asynchronous copy; the pinned buffer is reused only after the copy that last read it has completed (event), so
// uploading never waits for the kernels of the previous pass or frame.
struct PassTables {
    UploadRing<1> staging;      // pinned staging
    DevBuf d;                   // device arena
    std::vector<char> last;     // what the device arena holds: an unchanged object list is not uploaded again
    GeomParams gp;              // this pass's frame constants (kernel argument, by value)
    // device views into the arena (valid after upload)
    const ObjectRec *objs = nullptr;
    const uint32_t *vblock_obj = nullptr, *vblock_first = nullptr, *tblock_obj = nullptr, *tblock_first = nullptr;
    const float *vblock_bounds = nullptr, *tblock_bounds = nullptr;   // 6 floats per block (cluster_bounds)
};

struct Mesh {
    DevBuf d_vertices, d_indices;
    uint32_t n_vertices = 0, n_indices = 0;
    uint64_t material = 0;
    std::vector<float> tbounds, vbounds;   // cluster_bounds: 6 floats per block of SETUP_THREADS triangles / of 256 vertices
    // Skeletal skinning (arctic_set_mesh_skin / arctic_set_mesh_pose).  d_skin: one ArcticSkinVertex per vertex; while `posed`, d_posed -- a second
    // vertex buffer written by k_skin from d_vertices, d_skin and the pose's matrices in d_joints -- is what ObjectRec::vertices points at, and the
    // mesh's cluster boxes (which bound the bind pose) are replaced by infinite ones.  The matrices travel through a ring of pinned buffers, so
    // that a pose call neither reads the caller's memory after it returns nor waits for the copy of the pose before it.
    DevBuf d_skin;
    uint32_t n_joints = 0;
    DevBuf d_posed, d_joints;
    bool posed = false;
    static constexpr int POSE_RING = 3;
    UploadRing<POSE_RING> joints_ring;
    // Morph targets (arctic_set_mesh_morph_targets / arctic_set_mesh_morph_weights).  d_deltas: n_targets arrays of n_vertices records of 12 floats;
    // while `morphed` (some weight is not zero), d_morphed -- written by k_morph from d_vertices, d_deltas and the compacted {target, weight} list
    // in d_active -- is what k_skin reads if the mesh is posed and what ObjectRec::vertices points at if it is not.  The list travels through a
    // ring of pinned buffers like the joint matrices.  morph_weights: the weights in force (all zero after a targets call)
    DevBuf d_deltas, d_morphed;
    uint32_t n_targets = 0;
    DevBuf d_active;
    bool morphed = false;
    std::vector<float> morph_weights;
    UploadRing<POSE_RING> active_ring;
    uint64_t shape_seq = 0;   // bumped by every successful skin / pose / morph call: part of the shadow caches' keys (shadow_inputs, cube_inputs)
    const float *skin_input() const { return (morphed ? d_morphed : d_vertices).as<float>(); }          // morph first, then skin
    const float *vertices_in_use() const { return posed ? d_posed.as<float>() : skin_input(); }
    bool deformed() const { return posed || morphed; }                                                 // the cluster boxes do not describe it
    void release_morph() {    // (the caller has drained the streams that may read these)
        d_deltas.release(); d_morphed.release(); d_active.release(); active_ring.release();
        n_targets = 0; morphed = false; morph_weights.clear();
    }
    void release_pose() {     // (the caller has drained the streams that may read these)
        d_posed.release(); d_joints.release(); joints_ring.release();
        posed = false;
    }
    void release_skin() { release_pose(); d_skin.release(); n_joints = 0; }
};

}  // namespace arctic

using namespace arctic;   // (the handle is the C-ABI's type, so it is declared at global scope; every unit that includes this spells the project's names bare)

struct ArcticRenderer {
    int device = 0;
    hipStream_t stream = nullptr;       // the stream every pass is enqueued on (own_stream unless the caller set one); not owned
    uint32_t width = 0, height = 0, shadow_size = 0, max_lights = 0, row_begin = 0, row_end = 0;
    uint32_t tiles_x = 0, tiles_y = 0, tile_y0 = 0, row0_in_tile = 0;
    uint32_t band_rows = 0, shard_index = 0, shard_count = 1, owned_rows = 0;   // interleaved shard (band_rows > 0)
    std::vector<Mesh> meshes;
    std::vector<TexDesc> tex;        // 3 per material (device pointers)
    std::vector<DevBuf> tex_allocs;
    // arctic_set_material_extras: one entry per material.  While a material is not neutral (n_extras != 0) the device's texture table carries a
    // MaterialExtra record per material behind the descriptors (common.h) and every shading call takes the k_pbrlit* kernels (has_extras).
    struct Extras {
        float p[12] = {1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
        DevBuf d_emissive, d_occlusion, d_fast;   // plain RGBA8 images, or the one {e.rgb, o} image of the fast path
        uint32_t ew = 0, eh = 0, ow = 0, oh = 0;
        bool neutral = true;
    };
    std::vector<Extras> extras;
    uint32_t n_extras = 0;
    bool has_extras() const { return n_extras != 0; }
    DevBuf d_tex, d_lut, d_lights, d_light_pairs, d_env;
    // the shadow map, and the min/max of it per 4x4 texel block / per 4x4-aligned 8x8 block (k_shadow_bounds).  Two sets: a frame in
    // flight that redraws the map draws into the other one while the previous frame's shading still reads this one (the second set
    // is allocated when that first happens); `scur` names the map of the latest frame, the one every other call sees
    DevBuf d_shadow_set[2], d_shadow_blocks_set[2], d_shadow_bounds_set[2];
    bool bounds_valid_set[2] = {false, false};   // false whenever the map has been written since its table was built
    bool shadow_written_set[2] = {false, false}; // the map has been drawn (pass_shadow_map) or written (arctic_write_shadow_map): arctic_shade_hits asks
    int scur = 0;
    StreamMark shadow_set_released[2];   // like vis_set_released, for the shadow-map sets
    DevBuf &d_shadow() { return d_shadow_set[scur]; }
    DevBuf &d_shadow_blocks() { return d_shadow_blocks_set[scur]; }
    DevBuf &d_shadow_bounds() { return d_shadow_bounds_set[scur]; }
    bool &bounds_valid() { return bounds_valid_set[scur]; }
    uint32_t env_w = 0, env_h = 0;
    // ARCTIC_OPT_ENV_LIGHTING: the image-based ambient's tables (env_light.hip), built when the map and the option are both there
    int env_lighting = 0;
    bool env_built = false;          // the tables belong to the map in d_env
    DevBuf d_env_levels, d_env_lut, d_env_mips, d_env_sh_rows, d_env_tables;
    EnvTables env_host = {};         // the device struct's pointers and sizes (its sh[] is written by the device)
    bool env_active() const { return env_lighting == 1 && env_built; }
    uint32_t n_lights = 0;
    // arctic_update_spot_lights: SPOT_F4 float4 per light (common.h SpotDev); a non-empty list sends every tile to k_spotlit*
    DevBuf d_spots;
    uint32_t n_spots = 0;
    // arctic_update_point_shadow_lights: ONE allocation, n_cubes records (CUBE_F4 float4 each, common.h CubeDev) and behind them n_cubes x 6
    // faces of cube_size^2 floats; a non-empty list sends every tile to k_cubelit*.  One set of faces: they are drawn on the main stream,
    // behind the previous frame's shading that reads them (pass_point_shadows)
    DevBuf d_cubes;
    uint32_t n_cubes = 0, cube_size = 1024;         // cube_size: ARCTIC_OPT_POINT_SHADOW_SIZE
    bool cube_faces_filled = false;                 // the faces have been drawn (pass_point_shadows) or written (arctic_write_point_shadow) since the list or F was set: shade_hits asks under hit_model 1
    int hit_model = 0;                              // ARCTIC_OPT_HIT_MODEL: 0 = k_shade_hits, 1 = k_shade_hits_ext (hit_shade_ext.hip)
    std::vector<ArcticPointShadowLight> cube_lights;   // the list as given: the faces' matrices and the cache key
    std::vector<uint8_t> cube_key;                  // what the faces were drawn from (render_frame redraws them when it changes; empty: redraw)
    PinnedBuf cube_counts;                          // pinned, mapped: CUBE_COUNT_WORDS per face drawn (run_geometry's DepthTarget)
    uint32_t *h_cube_counts() const { return cube_counts.as<uint32_t>(); }
    uint32_t *dh_cube_counts() const { return cube_counts.dev<uint32_t>(); }
    uint32_t cube_count_faces = 0;
    // frame targets
    DevBuf d_vis_set[3], d_p0, d_p1, d_p2, d_p3, d_p4, d_rgba8, d_ldr, d_hdr, d_counter;
    bool have_gbuffer = false, have_output = false, have_vis = false;   // have_vis: d_vis holds the visibility of the current G-buffer
    bool hdr_valid = false;          // d_hdr holds the latest shading's colours: set where the shading pass is enqueued under ARCTIC_OPT_KEEP_FLOAT_OUTPUT, cleared by a resize and when the option is turned on (arctic_compose_planes_device asks)
    // ARCTIC_OPT_ANTIALIAS: with 1 a handle that owns the whole frame shades into d_rgba8 and the edge filter (antialias.hip) writes the
    // destination -- the caller's buffer or d_aa; output_filtered: the handle's latest RGBA8 output is the one in d_aa
    int antialias = 0;
    DevBuf d_aa;
    bool output_filtered = false;
    bool aa_active() const { return antialias == 1 && rows() == height; }
    const void *rgba8_output() const { return output_filtered ? d_aa.p : d_rgba8.p; }
    int light_path = 0;             // ARCTIC_OPT_LIGHT_PATH: 0 automatic, 1 scalar light loop, 2 packed pairs
    // ARCTIC_OPT_LIGHT_PAIR_RUNS: 1 = the pair table of the packed loop is laid out in runs that skip a colour channel (light_pair_table);
    // 0 = caller order, one general run.  h_lights: the lights as given, so that the option can rebuild the table; pair_runs: ShadeParams::pair_runs
    int light_pair_runs = 1;
    std::vector<ArcticPointLight> h_lights;
    uint32_t pair_runs = 0;
    bool visbuffer = true;          // arctic_render_frame shades straight from the visibility plane (no G-buffer)
    // per-frame geometry scratch
    PassTables tables[4];   // [0], [2], [3] forward pass (one per frame in flight), [1] shadow pass
    // transformed vertices, records, work items: one set per pass ([0] forward, [1] shadow), so that the two prepasses of a frame
    // can run side by side (arctic_render_frame) and the forward pass's records outlive a shadow pass (k_resolve, k_material_vis)
    struct GeoSet {
        DevBuf d_xverts, d_recs, d_rrecs, d_clip_list, d_rec_of, d_items;
        DevBuf d_left;                     // ... and the work items the bins did not take (same capacity as d_items), for the atomic rasteriser
        DevBuf d_bin_count, d_bin_slots;   // block ownership (common.h: BinTables): a counter and BIN_SLOTS record indices per 16x16 block of the target
        uint32_t item_cap = 0;      // entries of d_items (work-item table of the rasteriser)
        uint32_t bins_x = 0, bins_y = 0;   // blocks of the latest owned pass (arctic_read_bin_counts)
        uint32_t n_tblocks = 0, n_vblocks = 0; bool cull_counted = false;   // the latest pass's workgroups (arctic_read_cull_counts)
    } geo[4];   // indexed like tables
    DevBuf d_geo_counters, d_stage;
    // shadow_stream (below): arctic_render_frame draws the shadow map there while the main stream runs the visibility prepass
    // (the marks -- device_resources.h StreamMark -- keep the rules: never recorded or recorded on the waiting stream itself, nothing to wait for)
    StreamMark shadow_fork, shadow_drawn;
    // Skinning: k_skin runs on the main stream, which has joined every earlier prepass (prepass_done, shadow_drawn) -- so it follows every k_vertex that
    // still reads the buffer it overwrites.  `deformed` is recorded behind it; the shadow and prepass streams wait for it before their next pass,
    // once per recording (*_seen: the generation each of those streams has waited for)
    StreamMark deformed;
    uint64_t skin_seen_shadow = 0, skin_seen_prepass[2] = {0, 0};
    // The shadow pass has ONE set of scratch (geo[1], tables[1], its four counters) whichever stream it runs on -- the main stream
    // (arctic_pass_shadow_map, a sharded map, debug bit 7) or shadow_stream (whole frames).  shadow_scratch_free marks the end of the
    // last shadow pass; a pass on another stream waits for it first, so two never share the scratch.
    StreamMark shadow_scratch_free;
    // Frames in flight (arctic_render_frame, ARCTIC_OPT_FRAMES_IN_FLIGHT = 2): the visibility prepass of frame k + 1 runs on
    // prepass_stream while the main stream still shades frame k, so there are two sets of what the prepass writes and the
    // shading reads -- visibility plane, vertex / record / item tables, object tables -- and `cur` names the set of the latest frame
    // (the one the pass-level calls and arctic_read_gbuffer see).  vis_set_released[s]: everything enqueued on the main stream up to
    // the moment the handle moved on from set s; the next prepass into s waits for it.
    // Up to three sets (the reference keeps 3 frames in flight, rhi.hpp:25) and two prepass streams used alternately: with three
    // sets the prepasses of two consecutive frames are independent of each other as well, and a small frame -- whose prepass is a
    // chain of launches longer than its shading -- is bound by neither chain alone.
    int frames_in_flight = 2, frames_in_flight_opt = 0 /* ARCTIC_OPT_FRAMES_IN_FLIGHT; 0: by the target's size (alloc_targets) */, cur = 0, prepass_turn = 0;
    StreamMark prepass_done[2], vis_set_released[3];   // (prepass_stream[2]: below)
    DevBuf &d_vis() { return d_vis_set[cur]; }
    int fwd() const { return cur ? cur + 1 : 0; }      // index of the current forward set in tables / geo
    bool recs_worst_case = false;   // record table at 7 per source triangle (after an overflow of the 2-per-triangle table)
    uint32_t item_cap_floor = 1u << 22;   // its smallest size (ARCTIC_OPT_ITEM_TABLE_FLOOR; tests shrink it to reach the overflow path)
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t edge_stats[4] = {0, 0, 0, 0};   // stats[12..15]: fast tiles the shadow table left undecided, their undecided pixels, tiles / pixels that ran the 25 compares
    uint64_t light_stats[2] = {0, 0};   // stats[8], [9]: (tile, light) pairs with n.wi <= 0 in every lit lane; tiles with a lit pixel
    int keep_float = 0, count_evals = 0, culling = 1, debug = 0, hdr16 = 0, tile_trace = 0;
    uint32_t tiles_per_wave = 0;     // ARCTIC_OPT_TILES_PER_WAVE (0 = the library's default)
    // The shading pass's dispatch order (round 4): k_resolve leaves a cost class per tile next to the G-buffer (can a pixel of the tile be
    // lit at all?), k_tile_order turns the classes into the order in which arctic_pass_shade hands out its strips of 4 tiles.  A hint:
    // a stale or missing order changes the pass's time, never its image.
    DevBuf d_tile_class, d_order_lists, d_tile_order;
    bool have_order = false;         // d_tile_order belongs to the G-buffer in place
    uint32_t order_group = 0, order_slots = 0;   // ... built for this many tiles per wave, this many slots (common.h order_slot)
    int texture_tiling = -1;         // ARCTIC_OPT_TEXTURE_TILING: materials created from now on: -1 = 4 x 4-texel tiles for images of 2048 texels a side and more, 0 = never, 1 = always
    // ARCTIC_OPT_TEXTURE_MIPS: materials created under 1 get a chain (chains[m]: the host copy of the material's level descriptors, empty = one level);
    // at shading time 1 selects k_miplit* once a material has a chain.  d_lod: the level-of-detail plane next to the G-buffer (tile-major, allocated only
    // under the option); lod_valid: it belongs to the G-buffer in place (k_resolve_lod wrote it, or arctic_write_gbuffer / arctic_write_lod did)
    int texture_mips = 0;
    std::vector<std::vector<TexDesc>> chains;
    uint32_t n_chains = 0;
    DevBuf d_lod;
    bool lod_valid = false;
    bool mips_active() const { return texture_mips == 1 && n_chains != 0; }
    int sampler = 0;                 // ARCTIC_OPT_SAMPLER: bit 0 material footprints, bit 2 PCF taps with coordinates snapped to 1/256 texel (D3D-style 8-bit filter weights)
    int tile_order = 0;              // ARCTIC_OPT_TILE_ORDER: 0 (default since round 5) = the geometric, XCD-aware order of round 3; 1 = the cost-class order of round 4.
                                     // Measured (profiles/r5_a_*): the order gains <= 2 us of the pass, its one-workgroup kernel costs the G-buffer pass 112 us, and handing strips
                                     // out by cost instead of by XCD row costs the pass 83 MB of fabric reads per launch (L2 hits 2.33 M -> 1.73 M: neighbouring strips no longer meet in one L2)
    uint32_t order_tail = 60;        // ARCTIC_OPT_ORDER_TAIL: the last part of the order (per mille) that holds cheap strips only
    DevBuf d_tile_trace;             // ARCTIC_OPT_TILE_TRACE: 4 x u64 per tile of the latest shading pass
    int cluster_cull = 3;            // ARCTIC_OPT_CLUSTER_CULL: bit 0 k_setup skips clusters, bit 1 k_vertex skips vertex blocks, that cannot touch the pass's pixels
    int small_triangles = 1;         // ARCTIC_OPT_SMALL_TRIANGLES: 1 = the shadow pass's k_setup draws triangles with a small bounding box itself (geometry.hip: draw_small)
    int raster_owner = -1;           // ARCTIC_OPT_RASTER_OWNER: bit 0 forward pass, bit 1 shadow pass: the blocks of the target are written once by owner waves
                                     // (k_bin + k_raster_owned) instead of per-pixel atomics; -1: the library's choice
    uint32_t raster_blocks[2] = {2048, 2048};  // persistent grid of k_raster: [0] forward pass, [1] shadow pass
    // render_frame re-renders the shadow map only when its inputs changed (sun, objects, meshes): the reference redraws it
    // every frame (renderer.cpp:300-337), but a depth map of unchanged geometry from an unchanged light is the same map
    std::vector<uint8_t> shadow_key; bool shadow_cache = true;
    uint32_t cu_count = 256;
    // multi-GPU exchange (arctic_dist.h): an RCCL communicator owned by the handle, a communication stream ordered against the
    // main stream with events, the shard layout of every rank (all-gathered once at arctic_comm_init)
    Rccl::Comm comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    hipStream_t comm_stream = nullptr;   // the handle's own stream, borrowed, or comm_stream_owned (below)
    bool comm_stream_borrowed = false;   // the communication stream is the handle's own stream, idle because the caller brought its stream (one stream -- one hardware queue -- fewer)
    // ONE role per stream: own_stream is the main stream, or -- the caller brought its own -- EITHER the exchange's stream (borrowed by
    // arctic_comm_init) OR the second prepass stream of three frames in flight, never both: a gather queued in front of a prepass would
    // stall it behind the other ranks, and synchronising a prepass stream must never wait for an unmatched collective.
    bool own_stream_is_prepass() const { return stream != own_stream && !comm_stream_borrowed; }
    StreamMark shaded;                // the main stream, where a gather starts
    ReaderTable<4> shard_readers;     // gathers that still read a shard buffer
    std::vector<uint32_t> peer_rows, peer_ranges;    // rows of every rank's shard; [begin, end) of every rank (row-range shards)
    std::vector<uint64_t> peer_offset;               // byte offset of every rank's shard in the root's staging buffer (arctic_exchange_plan)
    uint64_t staging_bytes = 0;
    DevBuf d_staging, d_layout;                       // root: all shards back to back; ranges (2 u32 per rank) + byte offsets (u64 per rank)
    uint32_t layout_world = 0; bool layout_from_comm = false;
    bool shadow_sharded = false;                      // ARCTIC_OPT_SHADOW_SHARDED
    // Ray queries (arctic_trace_rays, arctic_trace_sun_visibility): the acceleration structure over the scene's world-space triangles, built on the
    // host (bvh.cpp) from the vertices in use, and cached: ray_key is what it was built from -- ray_inputs(), shadow_inputs' rule -- so a changed
    // object list, mesh count, pose or weights rebuilds it on the next query.  ray_tris: triangles stored (those that can be hit)
    struct RayScene {
        std::vector<uint8_t> key;
        bool built = false;
        uint64_t n_tris = 0, n_nodes = 0, builds = 0, depth = 0;
        DevBuf d_nodes, d_tris, d_rays, d_hits, d_mask;
        // ARCTIC_OPT_RAY_REFIT (ray_refit.hip; the definition: include/arctic_hip.h, "a refitted structure").  A full build under the option also
        // uploads the slots' sources and the refit's schedule (checked on the host first); while `refittable`, a change of the key that keeps the
        // objects' meshes (built_meshes) is followed on the device: a per-object table through a ring of pinned buffers, then one launch per stage,
        // all in stream order -- no synchronisation, nothing read back.  Nothing below is allocated while the option is 0
        int refit_opt = 0;
        bool refittable = false;
        uint64_t refits = 0, refit_launches = 0;
        std::vector<uint64_t> built_meshes;        // every object's mesh_idx at the build
        std::vector<uint32_t> stage_first;         // RefitSchedule::stage_first of the build
        DevBuf d_src, d_head, d_inputs, d_interior, d_objs;
        static constexpr int OBJ_RING = 3;
        UploadRing<OBJ_RING> objs_ring;
        // arctic_ray_scene_resplit (ray_resplit.hip; the definition: include/arctic_hip.h, "a re-split structure"): the sorts' workspace, allocated
        // by the first re-split of a structure of this size and kept; nothing while the call is never made
        DevBuf d_resplit;
        size_t resplit_bytes = 0;
        uint64_t resplit_slots = ~0ull;            // the slot count resplit_bytes was worked out for
        uint64_t resplits = 0, resplit_launches = 0, resplit_fell_back = 0;
        void drop() { built = false; refittable = false; key.clear(); }   // the cached structure is no longer the scene's: the next query builds
    } ray;
    // Ambient occlusion (arctic_trace_ambient_occlusion, ray_ao.hip): the direction table on the device -- at most 12 KiB, sent from a pinned copy
    // that is also what the device holds, so an unchanged table is not sent again and the pinned copy is rewritten only after the copy that last
    // read it has completed --, the hits plane and the result, one byte per pixel of the handle's rows each.  Nothing is allocated before the first call
    struct AmbientOcclusion {
        DevBuf d_dirs, d_hits, d_out;
        UploadRing<1> dirs_ring;                   // its one pinned slot keeps the table last sent
        size_t n_floats = 0;                       // what d_dirs holds (0: nothing)
    } ao;
    // Hit attributes (arctic_hit_attributes, hit_shade.hip): the prim-indexed source table -- where every triangle of the scene, in the ray queries'
    // numbering, takes its vertices from; it depends on the topology alone, so it is made again only behind a full build of the structure
    // (sources_of: RayScene::builds then) --, the per-object records of a call, which travel through a ring of pinned buffers like the refit's, and
    // the host forms' buffers.  Nothing is allocated before the first call of arctic_hit_attributes, arctic_shade_hits or arctic_trace_reflections
    struct HitScene {
        DevBuf d_src, d_objs, d_hits, d_attrs, d_material;
        DevBuf d_rays, d_color;                    // arctic_shade_hits' host form, and the reflection plane's rays, hits (d_hits) and result
        uint64_t n_prims = 0, sources_of = ~0ull, tables_made = 0;
        static constexpr int OBJ_RING = 3;
        UploadRing<OBJ_RING> objs_ring;
        size_t device_bytes() const { return d_src.cap + d_objs.cap + d_hits.cap + d_attrs.cap + d_material.cap + d_rays.cap + d_color.cap; }
        size_t pinned_bytes() const { size_t b = 0; for (const auto &s : objs_ring.slot) b += s.h.cap; return b; }
    } hit;
    // The composition (arctic_compose_planes_device, arctic_pass_ray_effects; compose.hip): the composed RGBA8, float LDR and float HDR of the handle's
    // rows.  Nothing is allocated before the first call that passes its checks.  pixels: rows * width of the latest composition (0: none; a resize
    // makes the handle's differ); own_rgba8: that call wrote d_rgba8, not the caller's buffer
    struct Compose {
        DevBuf d_rgba8, d_ldr, d_hdr;
        uint64_t pixels = 0, launches = 0, passes = 0;
        bool own_rgba8 = false;
        uint32_t flags = 0;   // the latest composition's (arctic_gi_compose_device asks whether it has scaled the ambient term already)
        size_t device_bytes() const { return d_rgba8.cap + d_ldr.cap + d_hdr.cap; }
    } compose;
    // The temporal accumulation of the occlusion plane (arctic_accumulate_ambient_occlusion_device; ao_history.hip): two sets of the two history
    // planes, tile-major like the G-buffer (n_tiles * 64 float4 each) -- a call reads set `cur` and writes the other, then `cur` moves.  Nothing is
    // allocated before the first call that passes its checks.  valid: H is not empty (cleared by arctic_ao_history_reset and by a resize);
    // proj_view, width, height: those of the call that wrote set `cur`
    struct AoHistory {
        DevBuf d_a[2], d_b[2];
        int cur = 0;
        bool valid = false;
        float proj_view[16] = {};
        uint32_t width = 0, height = 0;
        uint64_t launches = 0, calls = 0;
        size_t device_bytes() const { return d_a[0].cap + d_a[1].cap + d_b[0].cap + d_b[1].cap; }
    } ao_history;
    // Motion vectors (arctic_motion_vectors_device; motion.hip): the state M of include/arctic_hip.h -- what the previous motion call saw.  Per entry of
    // that call's object list its mesh and trs; that call's proj_view and frame size; per mesh (`shapes`, by mesh handle) where its vertices lay:
    // nothing for a mesh that was not deformed (its own buffer never changes), else a float4 snapshot written by k_motion_snapshot at the END of the
    // call that saw the pose, behind k_motion, which may still read the pose before it from the same buffer.  seq_at_call, rigid_at_call, seen_call:
    // the mesh's shape_seq, !deformed() and the call's number when a call last used the mesh.  The per-object table of a call travels through a
    // ring of pinned buffers like HitScene's.  d_pw .. d_src: the host form's planes; d_plane: the one call's.  `written`: recorded behind every
    // call, waited for by the next one if the handle's stream has changed in between.  Nothing is allocated before the first call that passes
    // its checks; valid: M is not empty (cleared by arctic_motion_reset and by a resize)
    struct Motion {
        struct PrevObject { uint64_t mesh; float trs[16]; };
        struct Shape {
            DevBuf d_snap;
            uint32_t n_vertices = 0;            // what d_snap holds room for
            uint64_t stamp = ~0ull;             // the shape_seq d_snap was written at (~0: never)
            uint64_t seq_at_call = 0, seen_call = 0;
            bool rigid_at_call = true;
        };
        bool valid = false;
        std::vector<PrevObject> objects;
        float proj_view[16] = {};
        uint32_t width = 0, height = 0;
        std::vector<Shape> shapes;
        DevBuf d_objs;
        static constexpr int OBJ_RING = 3;
        UploadRing<OBJ_RING> objs_ring;
        DevBuf d_pw, d_vel, d_bary, d_src, d_plane;
        StreamMark written;
        uint64_t launches = 0, snapshot_launches = 0, calls = 0, call_id = 0;
        size_t device_bytes() const {
            size_t b = d_objs.cap + d_pw.cap + d_vel.cap + d_bary.cap + d_src.cap + d_plane.cap;
            for (const Shape &s : shapes) b += s.d_snap.cap;
            return b;
        }
    } motion;
    // Temporal anti-aliasing (arctic_taa_resolve_device, arctic_set_camera_jitter; taa.hip): the state T of include/arctic_hip.h -- two sets of one
    // float4 plane {r, g, b, N}, tile-major like the G-buffer (n_tiles * 64 float4 each): a call reads set `cur` and writes the other, then `cur`
    // moves.  d_rgba8, d_ldr: the tonemapped result of the handle's rows; d_color, d_vel: the host form's planes, d_vel also arctic_pass_taa's
    // (its prev_world4 goes into Motion::d_plane).  `written`: recorded behind every call, waited for by the next one if the handle's stream has
    // changed in between.  Nothing is allocated before the first call that passes its checks; valid: T is not empty (cleared by
    // arctic_taa_reset and by a resize); width, height: those of the call that wrote set `cur`; own_rgba8: that call wrote d_rgba8, not the
    // caller's buffer.  jitter: arctic_set_camera_jitter's, in pixels -- host state alone, read by run_geometry's forward branch
    struct Taa {
        DevBuf d_t[2], d_rgba8, d_ldr, d_color, d_vel;
        int cur = 0;
        bool valid = false, own_rgba8 = false;
        bool by_pass = false;   // the call that wrote set `cur` was arctic_pass_taa: d_vel holds that frame's velocity2 (arctic_pass_motion_blur reads it)
        uint32_t width = 0, height = 0;
        float jitter[2] = {0.0f, 0.0f};
        StreamMark written;
        uint64_t launches = 0, calls = 0;
        size_t device_bytes() const { return d_t[0].cap + d_t[1].cap + d_rgba8.cap + d_ldr.cap + d_color.cap + d_vel.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && width == r.width && height == r.height; }   // the stage holds a result of the handle's frame size: the one spelling, on every stage below
    } taa;
    // Motion blur (arctic_motion_blur_device; motion_blur.hip): d_prep is P of include/arctic_hip.h (float2 per pixel, row-major), d_tile and
    // d_neighbour the two maxima (float2 per tile), d_hdr the blurred colour, d_rgba8 and d_ldr its tonemapped planes; d_color, d_vel, d_depth:
    // the host form's planes, d_vel and d_depth also arctic_pass_motion_blur's (its prev_world4 goes into Motion::d_plane).  `written`: recorded
    // behind every call, waited for by the next one if the handle's stream has changed in between.  Nothing is allocated before the first call
    // that passes its checks; valid: the planes hold a call's result at width x height (cleared by a resize); own_rgba8: that call wrote
    // d_rgba8, not the caller's buffer
    struct MotionBlur {
        DevBuf d_prep, d_tile, d_neighbour, d_hdr, d_rgba8, d_ldr, d_color, d_vel, d_depth;
        bool valid = false, own_rgba8 = false;
        uint32_t width = 0, height = 0;
        StreamMark written;
        uint64_t launches = 0, calls = 0;
        size_t device_bytes() const { return d_prep.cap + d_tile.cap + d_neighbour.cap + d_hdr.cap + d_rgba8.cap + d_ldr.cap + d_color.cap + d_vel.cap + d_depth.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && width == r.width && height == r.height; }
    } motion_blur;
    // Depth of field (arctic_dof_device; dof.hip): d_prep is P of include/arctic_hip.h (float2 per pixel, row-major), d_tile and d_neighbour
    // the two maxima (one float per tile), d_hdr the gathered colour, d_rgba8 and d_ldr its tonemapped planes; d_color, d_depth: the host
    // form's planes, d_depth also arctic_pass_dof's; d_taps: the tap table, which travels through taps_ring, whose one pinned slot keeps the
    // table last sent (n_taps float2; 0: nothing).  `written`: recorded behind every call, waited for by the next one if the handle's stream
    // has changed in between.  Nothing is allocated before the first call that passes its checks; valid: the planes hold a call's result at
    // width x height (cleared by a resize); own_rgba8: that call wrote d_rgba8, not the caller's buffer
    struct Dof {
        DevBuf d_prep, d_tile, d_neighbour, d_hdr, d_rgba8, d_ldr, d_color, d_depth, d_taps;
        UploadRing<1> taps_ring;
        uint32_t n_taps = 0;
        bool valid = false, own_rgba8 = false;
        uint32_t width = 0, height = 0;
        StreamMark written;
        uint64_t launches = 0, calls = 0;
        size_t device_bytes() const { return d_prep.cap + d_tile.cap + d_neighbour.cap + d_hdr.cap + d_rgba8.cap + d_ldr.cap + d_color.cap + d_depth.cap + d_taps.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && width == r.width && height == r.height; }
    } dof;
    // Bloom (arctic_bloom_device; bloom.hip, owned by bloom_calls.cpp): d_down and d_up are the two pyramids of include/arctic_hip.h as
    // arctic_bloom_layout packs them, sized for 8 levels whatever a call asks for; d_hdr the composite, d_rgba8 and d_ldr its tonemapped planes;
    // d_color: the host form's plane.  `written`: recorded behind every call, waited for by the next one if the handle's stream has changed in
    // between.  Nothing is allocated before the first call that passes its checks; valid: the planes hold a call's result at width x height
    // with `levels` levels (cleared by a resize); own_rgba8: that call wrote d_rgba8, not the caller's buffer
    struct Bloom {
        DevBuf d_down, d_up, d_hdr, d_rgba8, d_ldr, d_color;
        bool valid = false, own_rgba8 = false;
        uint32_t width = 0, height = 0, levels = 0;
        StreamMark written;
        uint64_t launches = 0, calls = 0;
        size_t device_bytes() const { return d_down.cap + d_up.cap + d_hdr.cap + d_rgba8.cap + d_ldr.cap + d_color.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && width == r.width && height == r.height; }
    } bloom;
    // Auto-exposure (arctic_exposure_device; exposure.hip, owned by exposure_calls.cpp): d_partials is the meter's table T[G][256] of
    // include/arctic_hip.h, d_hist the histogram H, d_state the 32-byte state record; d_hdr the exposed frame, d_rgba8 and d_ldr its tonemapped
    // planes (never allocated under ARCTIC_EXPOSURE_METER_ONLY); d_color: the host form's plane.  `written`: recorded behind every call, waited
    // for by the next one if the handle's stream has changed in between.  Nothing is allocated before the first call that passes its checks;
    // valid: d_state and d_hist hold a metering call's result at width x height (cleared by a resize and by arctic_exposure_reset: the next
    // resolve ignores what the record holds); planes: the output planes hold an applying call's; own_rgba8: that call wrote d_rgba8
    struct Exposure {
        DevBuf d_partials, d_hist, d_state, d_hdr, d_rgba8, d_ldr, d_color;
        bool valid = false, planes = false, own_rgba8 = false;
        uint32_t width = 0, height = 0;
        StreamMark written;
        uint64_t launches = 0, calls = 0, meters = 0;
        size_t device_bytes() const { return d_partials.cap + d_hist.cap + d_state.cap + d_hdr.cap + d_rgba8.cap + d_ldr.cap + d_color.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && width == r.width && height == r.height; }
    } exposure;
    // Volumetric fog (arctic_fog_device; fog.hip, owned by fog_calls.cpp): d_hdr is the fogged colour when the caller passes no HDR plane of its
    // own, d_rgba8 and d_ldr its tonemapped planes; d_color, d_depth: the host form's planes, d_depth also arctic_pass_fog's; d_offsets: the 16
    // offsets, which travel through offsets_ring, whose one pinned slot keeps the table last sent (have_offsets: it holds one).  `written`:
    // recorded behind every call, waited for by the next one if the handle's stream has changed in between.  Nothing is allocated before the
    // first call that passes its checks; valid: the planes hold a call's result at width x height (cleared by a resize); own_hdr, own_rgba8:
    // that call wrote d_hdr / d_rgba8, not the caller's planes
    struct Fog {
        DevBuf d_hdr, d_rgba8, d_ldr, d_color, d_depth, d_offsets;
        UploadRing<1> offsets_ring;
        bool have_offsets = false;
        bool valid = false, own_hdr = false, own_rgba8 = false;
        uint32_t width = 0, height = 0;
        StreamMark written;
        uint64_t launches = 0, calls = 0, uploads = 0;
        size_t device_bytes() const { return d_hdr.cap + d_rgba8.cap + d_ldr.cap + d_color.cap + d_depth.cap + d_offsets.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && width == r.width && height == r.height; }
    } fog;
    // Temporal upscaling (arctic_taa_upscale_device; taa_upscale.hip, owned by taa_upscale_calls.cpp): the state U of include/arctic_hip.h -- two
    // sets of one float4 plane {r, g, b, N} per OUTPUT pixel, tile-major in 8 x 8 output tiles: a call reads set `cur` and writes the other,
    // then `cur` moves.  d_rgba8, d_ldr: the tonemapped result at the output size; d_color, d_vel: the host form's input planes, d_vel also
    // arctic_pass_taa_upscale's (its prev_world4 goes into Motion::d_plane).  `written`: recorded behind every call, waited for by the next one
    // if the handle's stream has changed in between.  Nothing is allocated before the first call that passes its checks; valid: U is not empty
    // (cleared by arctic_taa_upscale_reset and by a resize); in_width, in_height, out_width, out_height: those of the call that wrote set
    // `cur`; own_rgba8: that call wrote d_rgba8, not the caller's buffer.  Apart from T: neither stage touches the other's state
    struct TaaUpscale {
        DevBuf d_u[2], d_rgba8, d_ldr, d_color, d_vel;
        int cur = 0;
        bool valid = false, own_rgba8 = false;
        uint32_t in_width = 0, in_height = 0, out_width = 0, out_height = 0;
        StreamMark written;
        uint64_t launches = 0, calls = 0;
        size_t device_bytes() const { return d_u[0].cap + d_u[1].cap + d_rgba8.cap + d_ldr.cap + d_color.cap + d_vel.cap; }
        bool holds(const ArcticRenderer &r) const { return valid && in_width == r.width && in_height == r.height; }   // ... at any output size
    } taa_upscale;
    // Indirect diffuse light (arctic_trace_gi; gi.hip, owned by gi_calls.cpp): the direction table on the device -- at most 3 KiB, sent from a
    // pinned copy that is also what the device holds, like the occlusion's --, the float4 sum S and the estimate E of the handle's rows.  The
    // rays, hits and colours of a round are HitScene's (the reflection plane's buffers), so a handle that traces both holds them once.  Nothing
    // is allocated before the first call that passes its checks.  pixels: rows * width of the latest estimate (0: none; a resize makes the
    // handle's differ); own_estimate: that call wrote d_estimate, not the caller's plane.  The accumulation (k_gi_accumulate): two sets of three
    // history planes, tile-major like the occlusion's (n_tiles * 64 float4 each, 96 bytes per pixel) -- a call reads set `hist_cur` and writes the
    // other, then it moves; hist_valid: the history is not empty (cleared by arctic_gi_history_reset and by a resize); proj_view, hist_width,
    // hist_height: those of the call that wrote set `hist_cur`.  The composition (k_gi_compose): d_hdr, d_ldr, d_rgba8 of the handle's rows;
    // composed: rows * width of the latest one; own_hdr, own_rgba8: it wrote the handle's planes, not the caller's
    struct Gi {
        DevBuf d_dirs, d_sum, d_estimate;
        UploadRing<1> dirs_ring;                   // its one pinned slot keeps the table last sent
        size_t n_floats = 0;                       // what d_dirs holds (0: nothing)
        uint64_t pixels = 0, launches = 0, calls = 0;
        bool own_estimate = false;
        DevBuf d_hist[2][3];
        int hist_cur = 0;
        bool hist_valid = false;
        float proj_view[16] = {};
        uint32_t hist_width = 0, hist_height = 0;
        uint64_t hist_calls = 0;
        DevBuf d_hdr, d_ldr, d_rgba8;
        uint64_t composed = 0, passes = 0;
        bool own_hdr = false, own_rgba8 = false;
        size_t history_bytes() const { size_t b = 0; for (const auto &set : d_hist) for (const DevBuf &d : set) b += d.cap; return b; }
        size_t device_bytes() const { return d_dirs.cap + d_sum.cap + d_estimate.cap + history_bytes() + d_hdr.cap + d_ldr.cap + d_rgba8.cap; }
    } gi;
    PinnedBuf counts;            // pinned, mapped: [0] records, [1] work items (forward), [2], [3] the same for the shadow pass, [4], [5] item-table overflow flags, [6], [7] work items drawn by the atomic rasteriser (forward, shadow)
    uint32_t *h_counts() const { return counts.as<uint32_t>(); }
    uint32_t *dh_counts() const { return counts.dev<uint32_t>(); }   // the device's address of h_counts
    // The streams the handle created, declared LAST: members are destroyed in reverse order, so every stream is waited for and gone before any
    // buffer, pinned slot or event above -- which its work may still touch -- is released.  (arctic_create makes them in the order its comment
    // gives; comm_stream_owned: the exchange's stream when it is not the borrowed own_stream.)
    Stream own_stream, shadow_stream, prepass_stream[2], comm_stream_owned;
    std::string err;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    uint32_t rows() const { return band_rows ? owned_rows : row_end - row_begin; }
    size_t n_tiles() const { return (size_t)tiles_x * tiles_y; }
    GBuffer gbuffer() const { return GBuffer{d_p0.as<float4>(), d_p4.as<float>(), d_p1.as<float4>(), d_p2.as<float4>(), d_p3.as<float4>()}; }
};

#define HIPCHECK(r, expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return (r)->fail(ARCTIC_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace arctic {

// Helpers that cross a unit boundary: defined in renderer.cpp, called from the other units as well (their comments are at the definitions).
// dir_from_rot and sun_proj_view, which the ray family also calls, are host_math.cpp's (common.h).
size_t shadow_alloc_bytes(const ArcticRenderer *r);
int select_device(ArcticRenderer *r);
int resolve_gbuffer(ArcticRenderer *r);
void put_objects(const ArcticRenderer *r, const ArcticScene *sc, std::vector<uint8_t> &k);
int check_item_overflow(ArcticRenderer *r);
bool valid_scene(const ArcticScene *sc);

// ... defined in ray_calls.cpp: the motion call behind its refusals, as arctic_pass_taa and arctic_pass_motion_blur make it; in
// motion_blur_calls.cpp: arctic_depth_plane_device behind its refusals, as arctic_pass_dof makes it
int motion_refusal(ArcticRenderer *r, const ArcticScene *sc, const void *prev_world4, const char *who);
int motion_planes(ArcticRenderer *r, const ArcticScene *sc, float4 *d_pw, float2 *d_vel, float *d_bary, uint4 *d_src);
int mb_depth_plane(ArcticRenderer *r, float *d_depth);
// ... defined in ray_calls.cpp as well, called by gi_calls.cpp (the indirect light is traced and shaded by the ray family's own steps): "the call
// needs a G-buffer" in its two steps, the structure of the ray queries for a scene, the sun's map as k_shade_hits needs it, the shading of n
// device rays and hits
int gbuffer_refusal(ArcticRenderer *r, const char *who);
int gbuffer_in_place(ArcticRenderer *r);
int ensure_ray_scene(ArcticRenderer *r, const ArcticScene *sc);
int sun_map_ready(ArcticRenderer *r, const char *who);
int shade_hits(ArcticRenderer *r, const ArcticScene *sc, const void *d_rays, const void *d_hits, uint64_t n, float4 *d_out);
// ... and why the frame's ambient term is not the flat ambient * base_color at level 0 that a correction of it assumes (null: it is)
const char *ambient_term_refusal(const ArcticRenderer *r);

// ... defined in post_source.cpp.  The planes a NULL colour pointer can mean to a post stage; each stage maps its own flag bits to one of them
enum class HdrSource { Shaded, Composed, Taa, MotionBlur, Dof, Bloom };
struct SourceFlag { HdrSource source; const char *flag; };   // flag: the public name of the flag that chose it, for the refusals' texts
struct SourcePlane { const void *color; bool color_taa; };   // color_taa: the history's tile-major float4 plane, not rows * width * 3 floats
int source_refusal(ArcticRenderer *r, SourceFlag s, const char *who);
int source_plane(ArcticRenderer *r, HdrSource source, SourcePlane &plane);
// the host forms' two ends
int upload_plane(ArcticRenderer *r, StreamMark &written, DevBuf &d, const void *plane, size_t px, size_t bytes_per_pixel);
constexpr bool FROM_FRAME = true;
int read_back(ArcticRenderer *r, void *out, const DevBuf &d, size_t bytes, bool from_frame = false);

}  // namespace arctic
