// exchange_calls.cpp -- the multi-GPU exchange of the C-ABI (include/arctic_dist.h): the plan as pure host functions, the RCCL communicator a handle
// owns, the gather of the shards' rows to a root and their placement in the frame (exchange.hip).  Of the handle (renderer_state.h) it owns the
// members from `comm` to `layout_from_comm`; the one user of RCCL outside it is the sharded shadow map's all-gather (renderer.cpp: pass_shadow_map).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "renderer_state.h"

namespace arctic {
Rccl g_rccl;
}  // namespace arctic

extern "C" {

// ---- multi-GPU exchange steps (include/arctic_dist.h) ------------------------------------------------------------------------
// the plan, as pure host functions (no device, no handle): everything below is built on them
int arctic_exchange_plan(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t world, const uint32_t *row_ranges,
                         uint32_t *rows, uint64_t *offset, uint64_t *total_bytes) {
    if (!rows || !offset || world == 0 || width == 0 || height == 0) return ARCTIC_E_INVALID;
    if (row_ranges) {
        if (band_rows) return ARCTIC_E_INVALID;
        for (uint32_t k = 0; k < world; ++k) {
            if (row_ranges[2 * k] > row_ranges[2 * k + 1] || row_ranges[2 * k + 1] > height) return ARCTIC_E_INVALID;
            rows[k] = row_ranges[2 * k + 1] - row_ranges[2 * k];
        }
    } else {
        if (!band_rows) return ARCTIC_E_INVALID;
        // band b -> rank b % world: full bands each, and the frame's last (possibly short) band to whoever it falls to
        const uint32_t n_bands = (height + band_rows - 1) / band_rows, last_rows = height - (n_bands - 1) * band_rows;
        for (uint32_t k = 0; k < world; ++k) {
            const uint32_t mine = n_bands / world + (k < n_bands % world ? 1u : 0u);
            rows[k] = mine * band_rows;
            if (mine && (n_bands - 1) % world == k) rows[k] -= band_rows - last_rows;
        }
    }
    uint64_t off = 0;
    for (uint32_t k = 0; k < world; ++k) { offset[k] = off; off += (uint64_t)rows[k] * width * 4; }
    if (total_bytes) *total_bytes = off;
    return ARCTIC_OK;
}

int arctic_exchange_row_source(uint32_t y, uint32_t height, uint32_t band_rows, uint32_t world, const uint32_t *row_ranges,
                               uint32_t *owner, uint32_t *local_row) {
    if (!owner || !local_row || world == 0 || y >= height || (!row_ranges && !band_rows) || (row_ranges && band_rows)) return ARCTIC_E_INVALID;
    return shard_row_source(y, band_rows, world, row_ranges, *owner, *local_row) ? 0 : 1;
}

int arctic_exchange_transfers(uint32_t width, uint32_t world, int32_t rank, int32_t root, const uint32_t *rows, const uint64_t *offset,
                              ArcticTransfer *out, uint32_t cap) {
    if (!rows || !offset || !out || world == 0 || rank < 0 || root < 0 || (uint32_t)rank >= world || (uint32_t)root >= world) return ARCTIC_E_INVALID;
    uint32_t n = 0;
    const uint64_t row_bytes = (uint64_t)width * 4;
    if (rank != root) {
        if (rows[rank]) { if (n >= cap) return ARCTIC_E_CAPACITY; out[n++] = ArcticTransfer{root, 1, 0, rows[rank] * row_bytes}; }
        return (int)n;
    }
    for (uint32_t k = 0; k < world; ++k) {
        if ((int32_t)k == root || !rows[k]) continue;
        if (n >= cap) return ARCTIC_E_CAPACITY;
        out[n++] = ArcticTransfer{(int32_t)k, 0, offset[k], rows[k] * row_bytes};
    }
    return (int)n;
}

namespace {

// rows of every rank's shard and where each shard starts in a staging buffer that holds them back to back; uploaded to d_layout
int upload_layout(ArcticRenderer *r, uint32_t world, const uint32_t *ranges /* 2 * world, or null: interleaved bands */, bool from_comm) {
    std::vector<uint32_t> rows(world, 0), rg(2 * (size_t)world, 0);
    std::vector<uint64_t> off(world, 0);
    uint64_t total = 0;
    if (ranges) std::memcpy(rg.data(), ranges, (size_t)world * 8);
    else if (!r->band_rows || r->shard_count != world) return r->fail(ARCTIC_E_INVALID, "frame layout: interleaved bands need band_rows > 0 and shard_count == world");
    if (arctic_exchange_plan(r->width, r->height, ranges ? 0u : r->band_rows, world, ranges, rows.data(), off.data(), &total) != ARCTIC_OK)
        return r->fail(ARCTIC_E_INVALID, "frame layout: bad row ranges");
    const size_t ranges_bytes = (((size_t)world * 8) + 15) / 16 * 16;
    HIPCHECK(r, r->d_layout.ensure(ranges_bytes + (size_t)world * 8));
    HIPCHECK(r, hipMemcpyAsync(r->d_layout.p, rg.data(), (size_t)world * 8, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, hipMemcpyAsync(r->d_layout.as<char>() + ranges_bytes, off.data(), (size_t)world * 8, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));   // the host vectors go out of scope
    r->peer_rows = rows; r->peer_offset = off; r->staging_bytes = total; r->peer_ranges = ranges ? rg : std::vector<uint32_t>();
    r->layout_world = world; r->layout_from_comm = from_comm;
    return ARCTIC_OK;
}
const uint32_t *layout_ranges(const ArcticRenderer *r) { return r->d_layout.as<uint32_t>(); }
const unsigned long long *layout_offsets(const ArcticRenderer *r) {
    return reinterpret_cast<const unsigned long long *>(r->d_layout.as<char>() + (((size_t)r->layout_world * 8) + 15) / 16 * 16);
}

// the second half of arctic_comm_init, free of RCCL calls (unit-testable through arctic_comm_init's error paths): `all` holds every
// rank's {row_begin, row_end, rows, band_rows}; checks them against this handle's sharding, uploads the layout, grows the shadow maps
int comm_adopt_layout(ArcticRenderer *r, const uint32_t *all, int world) {
    std::vector<uint32_t> ranges(2 * (size_t)world);
    for (int k = 0; k < world; ++k) {
        if (all[4 * k + 3] != r->band_rows) return r->fail(ARCTIC_E_INVALID, "comm_init: rank %d shards the frame differently (band_rows %u vs %u)", k, all[4 * k + 3], r->band_rows);
        ranges[2 * k] = all[4 * k]; ranges[2 * k + 1] = all[4 * k + 1];
    }
    int rc = upload_layout(r, (uint32_t)world, r->band_rows ? nullptr : ranges.data(), true);
    if (rc != ARCTIC_OK) return rc;
    for (int k = 0; k < world; ++k)
        if (r->peer_rows[(size_t)k] != all[4 * k + 2]) return r->fail(ARCTIC_E_INVALID, "comm_init: rank %d reports %u rows, the layout gives it %u", k, all[4 * k + 2], r->peer_rows[(size_t)k]);
    if (r->shadow_size) {   // room for the in-place all-gather of a sharded shadow map, in BOTH map sets (frames in flight flip between them)
        const size_t need = shadow_alloc_bytes(r);
        for (int s = 0; s < 2; ++s) {
            DevBuf &b = r->d_shadow_set[s];
            if (!b.p || b.cap >= need) continue;   // (the second set is allocated, at this size, when first used)
            HIPCHECK(r, hipStreamSynchronize(r->stream));
            HIPCHECK(r, b.ensure(need));
            HIPCHECK(r, launch_fill_u32(b.as<uint32_t>(), 0x3F800000u, (need - 8) / 4, r->stream));
            r->shadow_key.clear(); r->bounds_valid_set[s] = false; r->shadow_written_set[s] = false;
        }
    }
    return ARCTIC_OK;
}

}  // namespace

int arctic_comm_unique_id(void *id_out, char *err, uint64_t err_len) {
    auto say = [&](const char *m) { if (err && err_len) std::snprintf(err, (size_t)err_len, "%s", m); return ARCTIC_E_DEVICE; };
    if (!id_out) return ARCTIC_E_INVALID;
    if (!g_rccl.load()) return say("arctic_comm_unique_id: librccl.so could not be loaded");
    Rccl::UniqueId id;
    const int rc = g_rccl.GetUniqueId(&id);
    if (rc != 0) return say(g_rccl.why(rc));
    std::memcpy(id_out, id.internal, ARCTIC_COMM_ID_BYTES);
    return ARCTIC_OK;
}

int arctic_comm_init(ArcticRenderer *r, const void *id_bytes, int rank, int world) {
    if (!r) return ARCTIC_E_INVALID;
    if (!id_bytes || world < 1 || rank < 0 || rank >= world) return r->fail(ARCTIC_E_INVALID, "comm_init: bad id / rank / world");
    if (r->comm) return r->fail(ARCTIC_E_STATE, "comm_init: the handle already has a communicator");
    if (r->band_rows && ((uint32_t)world != r->shard_count || (uint32_t)rank != r->shard_index))
        return r->fail(ARCTIC_E_INVALID, "comm_init: rank %d of %d does not match the handle's shard %u of %u", rank, world, r->shard_index, r->shard_count);
    int rc = select_device(r);
    if (rc) return rc;
    if (!g_rccl.load()) return r->fail(ARCTIC_E_DEVICE, "comm_init: librccl.so could not be loaded");
    Rccl::UniqueId id;
    std::memcpy(id.internal, id_bytes, ARCTIC_COMM_ID_BYTES);
    int nrc = g_rccl.CommInitRank(&r->comm, world, id, rank);
    if (nrc != 0) { r->comm = nullptr; return r->fail(ARCTIC_E_DEVICE, "ncclCommInitRank: %s", g_rccl.why(nrc)); }
    r->comm_rank = rank; r->comm_world = world;
    // From here on the handle owns a communicator: any failure below gives it back (arctic_comm_destroy) before returning, so the
    // handle is never left half initialised (comm set, no layout) and arctic_comm_init can be called again.
    DevBuf tmp;
    const auto finish = [&]() -> int {
        if (!r->comm_stream) {
            // (the runtime deals few hardware queues to many streams, and two streams on one queue do not overlap: DESIGN.md 4.3)
            if (r->stream != r->own_stream) { r->comm_stream = r->own_stream; r->comm_stream_borrowed = true; }
            else { HIPCHECK(r, r->comm_stream_owned.create(hipStreamNonBlocking)); r->comm_stream = r->comm_stream_owned; }
        }
        HIPCHECK(r, r->shaded.ensure(hipEventDisableTiming));
        HIPCHECK(r, r->shard_readers.ensure(hipEventDisableTiming));
        // every rank's shard layout: {row_begin, row_end, rows, band_rows} all-gathered once (the root places shards of unequal size)
        HIPCHECK(r, tmp.ensure((size_t)world * 16));
        const uint32_t mine[4] = {r->band_rows ? 0u : r->row_begin, r->band_rows ? 0u : r->row_end, r->rows(), r->band_rows};
        HIPCHECK(r, hipMemcpyAsync(tmp.as<char>() + (size_t)rank * 16, mine, 16, hipMemcpyHostToDevice, r->comm_stream));
        const int arc = g_rccl.AllGather(tmp.as<char>() + (size_t)rank * 16, tmp.p, 4, Rccl::Uint32, r->comm, r->comm_stream);
        if (arc != 0) return r->fail(ARCTIC_E_DEVICE, "ncclAllGather(layout): %s", g_rccl.why(arc));
        std::vector<uint32_t> all((size_t)world * 4);
        HIPCHECK(r, hipMemcpyAsync(all.data(), tmp.p, (size_t)world * 16, hipMemcpyDeviceToHost, r->comm_stream));
        HIPCHECK(r, hipStreamSynchronize(r->comm_stream));
        return comm_adopt_layout(r, all.data(), world);
    };
    rc = finish();
    if (rc != ARCTIC_OK) {
        const std::string why = r->err;
        (void)arctic_comm_destroy(r);
        r->err = why;
        return rc;
    }
    return ARCTIC_OK;
}

int arctic_comm_destroy(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    if (r->comm_stream) (void)hipStreamSynchronize(r->comm_stream);
    if (r->comm) { (void)g_rccl.CommDestroy(r->comm); r->comm = nullptr; }
    r->comm_rank = 0; r->comm_world = 1;
    if (r->layout_from_comm) { r->layout_world = 0; r->layout_from_comm = false; }
    r->shard_readers.release();
    r->shaded.release();
    r->comm_stream_owned.release();   // (nothing when the stream was borrowed: own_stream stays the handle's)
    r->comm_stream = nullptr; r->comm_stream_borrowed = false;
    return ARCTIC_OK;
}

int arctic_gather_frame(ArcticRenderer *r, const void *d_shard, void *d_frame, int root) {
    if (!r) return ARCTIC_E_INVALID;
    if (!r->comm || !r->layout_from_comm) return r->fail(ARCTIC_E_STATE, "gather_frame: no communicator (arctic_comm_init)");
    if (root < 0 || root >= r->comm_world) return r->fail(ARCTIC_E_INVALID, "gather_frame: bad root");
    const bool is_root = r->comm_rank == root;
    if (is_root && !d_frame) return r->fail(ARCTIC_E_INVALID, "gather_frame: the root needs a frame buffer");
    if (!d_shard) {
        if (!r->have_output) return r->fail(ARCTIC_E_STATE, "gather_frame: no shaded output to gather");
        d_shard = r->rgba8_output();
    }
    int rc = select_device(r);
    if (rc) return rc;
    const size_t row_bytes = (size_t)r->width * 4;
    HIPCHECK(r, r->shaded.record(r->stream));        // after the shading that produced the shard ...
    HIPCHECK(r, r->shaded.wait(r->comm_stream));     // ... on the communication stream, beside the next frame
    const uint8_t *src = static_cast<const uint8_t *>(d_shard);
    if (r->comm_world > 1) {
        // the transfers of this rank, straight from the plan (arctic_exchange_transfers: what the CPU tests check for worlds 2..8)
        std::vector<ArcticTransfer> xfers((size_t)r->comm_world);
        const int n_x = arctic_exchange_transfers(r->width, (uint32_t)r->comm_world, r->comm_rank, root, r->peer_rows.data(), r->peer_offset.data(),
                                                  xfers.data(), (uint32_t)xfers.size());
        if (n_x < 0) return r->fail(ARCTIC_E_STATE, "gather_frame: no transfer plan");
        if (is_root) HIPCHECK(r, r->d_staging.ensure((size_t)r->staging_bytes));
        int nrc = g_rccl.GroupStart();
        if (nrc != 0) return r->fail(ARCTIC_E_DEVICE, "ncclGroupStart: %s", g_rccl.why(nrc));
        for (int i = 0; i < n_x && nrc == 0; ++i) {
            const ArcticTransfer &t = xfers[(size_t)i];
            nrc = t.is_send ? g_rccl.Send(src, (size_t)t.bytes, Rccl::Uint8, t.peer, r->comm, r->comm_stream)
                            : g_rccl.Recv(r->d_staging.as<char>() + t.staging_offset, (size_t)t.bytes, Rccl::Uint8, t.peer, r->comm, r->comm_stream);
        }
        const int erc = g_rccl.GroupEnd();
        if (nrc != 0 || erc != 0) return r->fail(ARCTIC_E_DEVICE, "ncclSend/ncclRecv(frame shards): %s", g_rccl.why(nrc ? nrc : erc));
        if (is_root) {
            HIPCHECK(r, hipMemcpyAsync(r->d_staging.as<char>() + r->peer_offset[(size_t)root], src, (size_t)r->rows() * row_bytes, hipMemcpyDeviceToDevice, r->comm_stream));
            src = r->d_staging.as<uint8_t>();
        }
    }
    if (is_root)
        HIPCHECK(r, launch_place_rows(src, static_cast<uint8_t *>(d_frame), r->width, r->height, r->band_rows, (uint32_t)r->comm_world,
                                      layout_ranges(r), layout_offsets(r), r->comm_stream));
    // whoever writes this shard buffer next waits for the transfers that still read it
    StreamMark *gathered = nullptr;
    HIPCHECK(r, r->shard_readers.claim(d_shard, r->comm_stream, gathered));
    HIPCHECK(r, gathered->record(r->comm_stream));
    return ARCTIC_OK;
}

int arctic_assemble_frame(ArcticRenderer *r, const void *d_staging, void *d_frame, uint32_t world, const uint32_t *row_ranges) {
    if (!r) return ARCTIC_E_INVALID;
    if (!d_staging || !d_frame || world == 0) return r->fail(ARCTIC_E_INVALID, "assemble_frame: null buffer or world == 0");
    int rc = select_device(r);
    if (rc) return rc;
    if (r->layout_from_comm && (uint32_t)r->comm_world != world) return r->fail(ARCTIC_E_STATE, "assemble_frame: the handle's communicator has another world size");
    if (!r->layout_from_comm && (rc = upload_layout(r, world, row_ranges, false)) != ARCTIC_OK) return rc;
    HIPCHECK(r, launch_place_rows(static_cast<const uint8_t *>(d_staging), static_cast<uint8_t *>(d_frame), r->width, r->height,
                                  row_ranges ? 0u : r->band_rows, world, layout_ranges(r), layout_offsets(r), r->stream));
    return ARCTIC_OK;
}

}  // extern "C"
