// resources_sanitize.cpp -- the owners of arctic-renderer_amd/csrc/device_resources.h over a fake HIP runtime, under -fsanitize=address,undefined, in a
// program of its own (tests/test_device_resources.py builds and runs it; it is never loaded into python and links no HIP library):
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/resources_sanitize.cpp
// The runtime functions the header calls are defined here as recorders over malloc / free: each logs its call, keeps the handles of its kind that are
// alive, and notes a release of a handle that is not.  The cases check the SEQUENCE of runtime calls each owner makes -- what the renderer's frame time
// and teardown depend on -- and that everything is released exactly once.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/device_resources.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace arctic;

namespace {
enum Kind { DEVICE, PINNED, EVENT, STREAM, N_KINDS };
struct Call { std::string fn; void *handle; size_t arg; void *stream; const void *src; };
std::vector<Call> calls;
std::set<void *> live[N_KINDS];
int double_releases = 0, refuse_device = 0, refuse_pinned = 0, refuse_alias = 0;

void *make(Kind k, size_t bytes) { void *p = std::malloc(bytes ? bytes : 1); live[k].insert(p); return p; }
void drop(Kind k, void *p) { if (live[k].erase(p)) std::free(p); else ++double_releases; }
bool refused(int &n) { if (n > 0) { --n; return true; } return false; }
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) {
    if (refused(refuse_device)) { calls.push_back({"hipMalloc!", nullptr, n, nullptr, nullptr}); return hipErrorOutOfMemory; }
    *p = make(DEVICE, n); calls.push_back({"hipMalloc", *p, n, nullptr, nullptr}); return hipSuccess;
}
hipError_t hipFree(void *p) { calls.push_back({"hipFree", p, 0, nullptr, nullptr}); drop(DEVICE, p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags) {
    if (refused(refuse_pinned)) { calls.push_back({"hipHostMalloc!", nullptr, n, nullptr, nullptr}); return hipErrorOutOfMemory; }
    *p = make(PINNED, n); calls.push_back({"hipHostMalloc", *p, n, reinterpret_cast<void *>((size_t)flags), nullptr}); return hipSuccess;
}
hipError_t hipHostFree(void *p) { calls.push_back({"hipHostFree", p, 0, nullptr, nullptr}); drop(PINNED, p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) {
    calls.push_back({"hipHostGetDevicePointer", h, 0, nullptr, nullptr});
    if (refused(refuse_alias)) return hipErrorInvalidValue;
    *d = h; return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { *e = static_cast<hipEvent_t>(make(EVENT, 1)); calls.push_back({"hipEventCreateWithFlags", *e, flags, nullptr, nullptr}); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { calls.push_back({"hipEventDestroy", e, 0, nullptr, nullptr}); drop(EVENT, e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { calls.push_back({"hipEventRecord", e, 0, s, nullptr}); return live[EVENT].count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t e) { calls.push_back({"hipEventSynchronize", e, 0, nullptr, nullptr}); return live[EVENT].count(e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t s) {
    calls.push_back({"hipMemcpyAsync", dst, n, s, src}); std::memcpy(dst, src, n); return hipSuccess;   // (a real copy: the sanitizer sees a slot or a destination that is too small)
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { *s = static_cast<hipStream_t>(make(STREAM, 1)); calls.push_back({"hipStreamCreateWithFlags", *s, flags, nullptr, nullptr}); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { calls.push_back({"hipStreamSynchronize", s, 0, s, nullptr}); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { calls.push_back({"hipStreamDestroy", s, 0, nullptr, nullptr}); drop(STREAM, s); return hipSuccess; }
}

namespace {
int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("BAD %s: line %d: %s\n", name, __LINE__, #cond); ++failures; return; } } while (0)
size_t alive() { size_t n = 0; for (auto &s : live) n += s.size(); return n; }
// the names of the calls made since `from`, space separated
std::string since(size_t from) { std::string t; for (size_t i = from; i < calls.size(); ++i) t += (t.empty() ? "" : " ") + calls[i].fn; return t; }
void done(const char *name) { std::printf("ok %s\n", name); }

void dev_buf() {
    const char *name = "devbuf-ensure-and-exact";
    {
        DevBuf b;
        size_t at = calls.size();
        CHECK(b.ensure(100) == hipSuccess && since(at) == "hipMalloc" && calls.back().arg == 100 + 25 + 256 && b.cap == 381 && b.p);
        at = calls.size();
        CHECK(b.ensure(50) == hipSuccess && b.ensure(381) == hipSuccess && b.ensure(0) == hipSuccess && calls.size() == at);
        void *old = b.p;
        CHECK(b.ensure(382) == hipSuccess && since(at) == "hipFree hipMalloc" && calls[at].handle == old && calls.back().arg == 382 + 95 + 256 && b.cap == 733);
        DevBuf x;
        at = calls.size();
        CHECK(x.alloc_exact(1000) == hipSuccess && since(at) == "hipMalloc" && calls.back().arg == 1000 && x.cap == 1000 && x.as<char>() == x.p);
        at = calls.size();
        x.release(); x.release();
        CHECK(since(at) == "hipFree" && !x.p && x.cap == 0 && !x);
        DevBuf moved = std::move(b);
        CHECK(!b.p && b.cap == 0 && moved.cap == 733);
        moved = DevBuf();   // move assignment releases what it held
        CHECK(!moved.p && live[DEVICE].empty());
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

void ring_of_three() {
    const char *name = "ring3-seven-uploads";
    hipStream_t stream = reinterpret_cast<hipStream_t>(&failures);   // (never dereferenced: the ring only passes it on)
    std::vector<char> dst(64);
    {
        UploadRing<3> ring;
        void *host_of[3] = {nullptr, nullptr, nullptr};
        hipEvent_t event_of[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < 7; ++i) {
            const int slot = i % 3;
            CHECK(ring.turn == slot);
            size_t at = calls.size();
            char *h = nullptr;
            CHECK(ring.stage(64, &h) == hipSuccess && h);
            if (i < 3) {   // a slot is made on its first use, and nothing is waited for
                CHECK(since(at) == "hipHostMalloc hipEventCreateWithFlags" && calls[at].arg == 64 && calls[at + 1].arg == hipEventDisableTiming);
                host_of[slot] = h; event_of[slot] = static_cast<hipEvent_t>(calls[at + 1].handle);
                for (int k = 0; k < slot; ++k) CHECK(host_of[k] != h);
            } else {       // its copy is pending: its own event is waited for before the memory is handed out again, and nothing else happens
                CHECK(since(at) == "hipEventSynchronize" && calls[at].handle == event_of[slot] && h == host_of[slot]);
            }
            std::memset(h, i + 1, 64);
            at = calls.size();
            CHECK(ring.send(dst.data(), 64, stream) == hipSuccess && since(at) == "hipMemcpyAsync hipEventRecord");
            CHECK(calls[at].src == h && calls[at].handle == dst.data() && calls[at].arg == 64 && calls[at].stream == stream);
            CHECK(calls[at + 1].handle == event_of[slot] && calls[at + 1].stream == stream && ring.slot[slot].pending && dst[63] == i + 1);
        }
        CHECK(ring.turn == 1 && live[PINNED].size() == 3 && live[EVENT].size() == 3);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

void ring_of_one() {
    const char *name = "ring1-waits-only-when-pending";
    std::vector<char> dst(256);
    {
        UploadRing<1> ring;
        char *h = nullptr;
        CHECK(ring.stage(64, &h) == hipSuccess && ring.send(dst.data(), 64, nullptr) == hipSuccess && ring.turn == 0);
        size_t at = calls.size();
        CHECK(ring.stage(64, &h) == hipSuccess && since(at) == "hipEventSynchronize");      // after a send: waits
        at = calls.size();
        CHECK(ring.stage(64, &h) == hipSuccess && ring.stage(10, &h) == hipSuccess && calls.size() == at);   // no send since the wait: nothing
        at = calls.size();
        CHECK(ring.send(dst.data(), 0, nullptr) == hipSuccess && calls.size() == at && !ring.slot[0].pending);   // nothing to send: no call, not pending
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
    name = "ring-slot-grows-and-is-kept";
    {
        UploadRing<3> ring;
        char *h = nullptr;
        CHECK(ring.stage(64, &h) == hipSuccess && ring.send(dst.data(), 64, nullptr) == hipSuccess);
        CHECK(ring.send(dst.data(), 0, nullptr) == hipSuccess && ring.send(dst.data(), 0, nullptr) == hipSuccess && ring.turn == 0);   // an empty upload moves the ring on
        void *small = h;
        hipEvent_t ev = ring.slot[0].copied;
        size_t at = calls.size();
        CHECK(ring.stage(128, &h) == hipSuccess && since(at) == "hipEventSynchronize hipHostFree hipHostMalloc");   // asked for more: waited for, freed, made again
        CHECK(calls[at + 1].handle == small && calls[at + 2].arg == 128 && ring.slot[0].h.cap == 128 && ring.slot[0].copied == ev);
        std::memset(h, 7, 128);
        CHECK(ring.send(dst.data(), 128, nullptr) == hipSuccess);
        (void)ring.send(dst.data(), 0, nullptr); (void)ring.send(dst.data(), 0, nullptr);
        void *big = h;
        at = calls.size();
        CHECK(ring.stage(32, &h) == hipSuccess && since(at) == "hipEventSynchronize" && h == big && ring.slot[0].h.cap == 128);   // asked for less: kept
        at = calls.size();
        ring.release();
        CHECK(since(at) == "hipHostFree hipEventDestroy" && ring.turn == 0 && !ring.slot[0].pending);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

struct Holder { DevBuf d; PinnedBuf p; Event e; UploadRing<3> ring; int tag = 0; };

void moved_in_a_vector() {
    const char *name = "move-vector-growth";
    std::vector<char> dst(64);
    {
        std::vector<Holder> v(1);
        char *h = nullptr;
        size_t at = calls.size();
        CHECK(v[0].p.alloc(64, hipHostMallocMapped) == hipSuccess && since(at) == "hipHostMalloc hipHostGetDevicePointer" && v[0].p.dev<char>() == v[0].p.as<char>());
        CHECK(v[0].d.ensure(100) == hipSuccess && v[0].e.create(hipEventDisableTiming) == hipSuccess);
        at = calls.size();
        CHECK(v[0].e.ensure(hipEventDisableTiming) == hipSuccess && calls.size() == at);   // created already: nothing
        CHECK(v[0].ring.stage(64, &h) == hipSuccess && v[0].ring.send(dst.data(), 64, nullptr) == hipSuccess);
        v[0].tag = 42;
        void *d = v[0].d.p, *p = v[0].p.p;
        hipEvent_t e = v[0].e;
        const size_t n_calls = calls.size(), n_alive = alive(), n_dev = live[DEVICE].size(), n_pin = live[PINNED].size(), n_ev = live[EVENT].size();
        const Holder *first = v.data();
        while (v.size() < 9) v.emplace_back();
        CHECK(v.data() != first);                                     // the elements did move
        CHECK(calls.size() == n_calls);                               // ... without a runtime call
        CHECK(v[0].tag == 42 && v[0].d.p == d && v[0].d.cap == 381 && v[0].p.p == p && v[0].p.d == p && v[0].p.cap == 64 && v[0].e == e);
        CHECK(v[0].ring.turn == 1 && v[0].ring.slot[0].pending && v[0].ring.slot[0].h.p == h && !v[0].ring.slot[1].pending);
        CHECK(alive() == n_alive && live[DEVICE].size() == n_dev && live[PINNED].size() == n_pin && live[EVENT].size() == n_ev);
        at = calls.size();
        CHECK(v[0].ring.send(dst.data(), 0, nullptr) == hipSuccess && v[0].ring.send(dst.data(), 0, nullptr) == hipSuccess);
        CHECK(v[0].ring.stage(64, &h) == hipSuccess && since(at) == "hipEventSynchronize");   // the pending slot is still waited for after the move
        v.clear();
        CHECK(alive() == 0);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

void refused_allocations() {
    const char *name = "failed-allocation-leaves-empty";
    {
        DevBuf b;
        refuse_device = 1;
        CHECK(b.ensure(100) == hipErrorOutOfMemory && !b.p && b.cap == 0);
        CHECK(b.ensure(100) == hipSuccess && b.cap == 381);
        refuse_device = 1;
        CHECK(b.ensure(1000) == hipErrorOutOfMemory && !b.p && b.cap == 0 && live[DEVICE].empty());   // (what it held went first, as ever)
        refuse_device = 1;
        CHECK(b.alloc_exact(10) == hipErrorOutOfMemory && !b.p && b.alloc_exact(10) == hipSuccess && b.cap == 10);
        PinnedBuf p;
        refuse_pinned = 1;
        CHECK(p.alloc(64, hipHostMallocDefault) == hipErrorOutOfMemory && !p.p && p.cap == 0);
        refuse_alias = 1;
        CHECK(p.alloc(64, hipHostMallocMapped) == hipErrorInvalidValue && !p.p && !p.d && live[PINNED].empty());
        CHECK(p.alloc(64, hipHostMallocMapped) == hipSuccess && p.p && p.d);
        UploadRing<1> ring;
        char *h = nullptr;
        refuse_pinned = 1;
        CHECK(ring.stage(64, &h) == hipErrorOutOfMemory && !h && !ring.slot[0].h.p && !ring.slot[0].pending);
        CHECK(ring.stage(64, &h) == hipSuccess && h);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

void streams_and_events() {
    const char *name = "stream-waits-then-goes-once";
    {
        Stream s, none;
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && calls.back().arg == hipStreamNonBlocking);
        hipStream_t raw = s;
        Stream t = std::move(s);   // the hand-over of arctic_use_own_stream
        CHECK(!s && t == raw);
        size_t at = calls.size();
        s.release(); none.release();
        CHECK(calls.size() == at);
        t.release();
        CHECK(since(at) == "hipStreamSynchronize hipStreamDestroy" && calls[at].handle == raw && !t);
        Event e, f;
        CHECK(e.ensure(0) == hipSuccess && f.create(hipEventDisableTiming) == hipSuccess && live[EVENT].size() == 2);
        f = std::move(e);
        CHECK(live[EVENT].size() == 1 && !e);
        Stream kept;
        CHECK(kept.create(hipStreamNonBlocking) == hipSuccess);
    }
    CHECK(alive() == 0 && double_releases == 0 && since(calls.size() - 3) == "hipStreamSynchronize hipStreamDestroy hipEventDestroy");   // a scope's end does the same
    done(name);
}
}  // namespace

int main() {
    dev_buf();
    ring_of_three();
    ring_of_one();
    moved_in_a_vector();
    refused_allocations();
    streams_and_events();
    const char *name = "all-released-once";
    if (alive() != 0 || double_releases != 0) { std::printf("BAD %s: %zu handles alive, %d released twice\n", name, alive(), double_releases); ++failures; }
    else done(name);
    return failures ? 1 : 0;
}
