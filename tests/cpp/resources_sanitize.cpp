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
int double_releases = 0, refuse_device = 0, refuse_pinned = 0, refuse_alias = 0, refuse_wait = 0;

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
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) {
    if (refused(refuse_wait)) { calls.push_back({"hipStreamWaitEvent!", e, flags, s, nullptr}); return hipErrorInvalidValue; }
    calls.push_back({"hipStreamWaitEvent", e, flags, s, nullptr}); return live[EVENT].count(e) ? hipSuccess : hipErrorInvalidHandle;
}
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

struct Holder { DevBuf d; PinnedBuf p; Event e; UploadRing<3> ring; StreamMark mark; ReaderTable<4> readers; int tag = 0; };

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
        hipStream_t on = reinterpret_cast<hipStream_t>(&failures);
        StreamMark *claimed = nullptr;
        CHECK(v[0].mark.create(hipEventDisableTiming) == hipSuccess && v[0].mark.record(on) == hipSuccess);
        CHECK(v[0].readers.ensure(hipEventDisableTiming) == hipSuccess && v[0].readers.claim(dst.data(), nullptr, claimed) == hipSuccess && claimed->record(on) == hipSuccess);
        const hipEvent_t mark_ev = v[0].mark.ev, reader_ev = claimed->ev;
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
        CHECK(v[0].mark.ev == mark_ev && v[0].mark.recorded && v[0].mark.on == on && v[0].mark.generation == 1);
        CHECK(v[0].readers.slot[0].ptr == dst.data() && v[0].readers.slot[0].done.ev == reader_ev && v[0].readers.slot[0].done.recorded && !v[0].readers.slot[1].ptr);
        CHECK(alive() == n_alive && live[DEVICE].size() == n_dev && live[PINNED].size() == n_pin && live[EVENT].size() == n_ev);
        at = calls.size();
        CHECK(v[0].ring.send(dst.data(), 0, nullptr) == hipSuccess && v[0].ring.send(dst.data(), 0, nullptr) == hipSuccess);
        CHECK(v[0].ring.stage(64, &h) == hipSuccess && since(at) == "hipEventSynchronize");   // the pending slot is still waited for after the move
        at = calls.size();
        CHECK(v[0].mark.wait(nullptr) == hipSuccess && v[0].readers.wait_for(dst.data(), nullptr) == hipSuccess && since(at) == "hipStreamWaitEvent hipStreamWaitEvent");
        CHECK(calls[at].handle == mark_ev && calls[at + 1].handle == reader_ev);   // the mark and the claimed slot are still waited for after the move
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

// two streams that exist (the default stream, nullptr, is the third one the cases use)
struct TwoStreams {
    Stream a, b;
    bool make() { return a.create(hipStreamNonBlocking) == hipSuccess && b.create(hipStreamNonBlocking) == hipSuccess; }
};
bool waited(size_t at, hipStream_t stream, hipEvent_t ev) {   // exactly one call since `at`: `stream` waits for `ev`
    return calls.size() == at + 1 && calls[at].fn == "hipStreamWaitEvent" && calls[at].stream == stream && calls[at].handle == ev && calls[at].arg == 0;
}

void marks() {
    const char *name = "mark-never-recorded-never-waited-for";
    {
        TwoStreams s;
        StreamMark m, empty;
        uint64_t seen = 0;
        CHECK(s.make() && m.create(hipEventDisableTiming) == hipSuccess && calls.back().fn == "hipEventCreateWithFlags" && calls.back().arg == hipEventDisableTiming);
        size_t at = calls.size();
        CHECK(m.wait(s.a) == hipSuccess && m.wait(nullptr) == hipSuccess && m.wait_once(s.a, seen) == hipSuccess && m.wait_once(nullptr, seen) == hipSuccess);
        CHECK(empty.wait(s.a) == hipSuccess && empty.wait_once(nullptr, seen) == hipSuccess);
        CHECK(calls.size() == at && seen == 0 && !m.recorded && m.generation == 0);
        CHECK(m.ensure(hipEventDisableTiming) == hipSuccess && calls.size() == at);   // created already: nothing
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
    name = "mark-same-stream-elided-others-wait";
    {
        TwoStreams s;
        CHECK(s.make());
        const hipStream_t recorded_on[2] = {nullptr, s.a};   // the default stream is a stream like any other
        for (hipStream_t on : recorded_on) {
            StreamMark m;
            CHECK(m.create(hipEventDisableTiming) == hipSuccess);
            size_t at = calls.size();
            CHECK(m.record(on) == hipSuccess && since(at) == "hipEventRecord" && calls[at].handle == m.ev.e && calls[at].stream == on);
            CHECK(m.recorded && m.on == on && m.generation == 1);
            at = calls.size();
            CHECK(m.wait(on) == hipSuccess && calls.size() == at);                    // same stream: stream order does it
            CHECK(m.wait(s.b) == hipSuccess && waited(at, s.b, m.ev));
            const hipStream_t other = on ? nullptr : static_cast<hipStream_t>(s.a);
            at = calls.size();
            CHECK(m.wait(other) == hipSuccess && waited(at, other, m.ev));
            at = calls.size();                                                        // two passes on one stream, then one on another (the shadow scratch)
            CHECK(m.wait(on) == hipSuccess && m.record(on) == hipSuccess && m.wait(on) == hipSuccess && m.record(on) == hipSuccess && since(at) == "hipEventRecord hipEventRecord");
            CHECK(m.wait(s.b) == hipSuccess && m.record(s.b) == hipSuccess && since(at + 2) == "hipStreamWaitEvent hipEventRecord" && calls[at + 2].stream == s.b && m.on == s.b);
            at = calls.size();
            CHECK(m.wait(s.b) == hipSuccess && calls.size() == at && m.wait(on) == hipSuccess && waited(at, on, m.ev));
        }
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
    name = "mark-forget";
    {
        TwoStreams s;
        StreamMark m;
        CHECK(s.make() && m.create(0) == hipSuccess && m.record(s.a) == hipSuccess);
        const hipEvent_t ev = m.ev;
        size_t at = calls.size();
        m.forget();
        CHECK(m.wait(s.b) == hipSuccess && m.wait(nullptr) == hipSuccess && calls.size() == at && m.ev == ev && m.generation == 1);   // no runtime call, the event is kept
        CHECK(m.record(nullptr) == hipSuccess && m.generation == 2);
        at = calls.size();
        CHECK(m.wait(nullptr) == hipSuccess && calls.size() == at && m.wait(s.b) == hipSuccess && waited(at, s.b, ev));
        at = calls.size();
        m.release();                                                                   // release forgets as well
        CHECK(since(at) == "hipEventDestroy" && !m.recorded && !m.ev && m.wait(s.b) == hipSuccess && calls.size() == at + 1);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
    name = "mark-generations";
    {
        TwoStreams s;
        StreamMark m;
        uint64_t seen_a = 0, seen_b = 0;
        CHECK(s.make() && m.create(hipEventDisableTiming) == hipSuccess);
        for (uint64_t g = 1; g <= 3; ++g) {   // each waiter waits once per record, however often it asks
            CHECK(m.record(nullptr) == hipSuccess && m.generation == g);
            size_t at = calls.size();
            CHECK(m.wait_once(s.a, seen_a) == hipSuccess && waited(at, s.a, m.ev) && seen_a == g);
            CHECK(m.wait_once(s.a, seen_a) == hipSuccess && calls.size() == at + 1);
            if (g == 2) continue;             // waiter b misses a generation: it waits once for the latest
            at = calls.size();
            CHECK(m.wait_once(s.b, seen_b) == hipSuccess && waited(at, s.b, m.ev) && seen_b == g);
            CHECK(m.wait_once(s.b, seen_b) == hipSuccess && m.wait_once(s.a, seen_a) == hipSuccess && calls.size() == at + 1);
        }
        seen_b = 0;                           // the waiter is another stream now (arctic_set_stream): it waits again, once
        size_t at = calls.size();
        CHECK(m.wait_once(s.b, seen_b) == hipSuccess && waited(at, s.b, m.ev) && seen_b == 3 && m.wait_once(s.b, seen_b) == hipSuccess && calls.size() == at + 1);
        refuse_wait = 1;                      // a refused wait leaves `seen` as it was: the next call waits again
        CHECK(m.record(nullptr) == hipSuccess);
        at = calls.size();
        CHECK(m.wait_once(s.a, seen_a) == hipErrorInvalidValue && seen_a == 3 && since(at) == "hipStreamWaitEvent!");
        at = calls.size();
        CHECK(m.wait_once(s.a, seen_a) == hipSuccess && waited(at, s.a, m.ev) && seen_a == 4);
        seen_a = 0;                           // a waiter on the recording stream itself: nothing to wait for, and it has seen the generation
        at = calls.size();
        CHECK(m.wait_once(nullptr, seen_a) == hipSuccess && calls.size() == at && seen_a == 4);
        StreamMark never;                     // a waiter reset to 0 waits again only if something was ever recorded
        uint64_t seen = 0;
        CHECK(never.create(0) == hipSuccess);
        at = calls.size();
        CHECK(never.wait_once(s.a, seen) == hipSuccess && calls.size() == at && seen == 0);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

// the sets of frames in flight.  A frame enters set k % 3 (its prepass stream waits for the set's mark) and leaves it when the next frame starts
// (the main stream records the mark): renderer.cpp's "record the set left, advance, wait on the set entered" with the frame's own record put
// first.  (The renderer's very first frame also records the set it starts in, which no frame has drawn into.)
void ring_of_marks() {
    const char *name = "mark-ring-of-three-sets";
    {
        TwoStreams s;
        Stream main_stream;
        StreamMark released[3];
        CHECK(s.make() && main_stream.create(hipStreamNonBlocking) == hipSuccess);
        for (StreamMark &m : released) CHECK(m.create(hipEventDisableTiming) == hipSuccess);
        size_t record_of[3] = {0, 0, 0};   // index in `calls` of the set's latest record
        for (int pass = 0; pass < 2; ++pass) {
            for (int frame = 0; frame < (pass ? 3 : 7); ++frame) {
                const int set = frame % 3;
                const hipStream_t ps = frame & 1 ? s.b : s.a;
                size_t at = calls.size();
                CHECK(released[set].wait(ps) == hipSuccess);
                if (frame < 3) CHECK(calls.size() == at);   // nothing has left this set (again, after forget): nothing to wait for
                else {
                    CHECK(waited(at, ps, released[set].ev));
                    // the mark's latest record is the one made when this set was left three frames earlier, and nothing has been recorded on it since
                    CHECK(calls[record_of[set]].fn == "hipEventRecord" && calls[record_of[set]].handle == released[set].ev.e && released[set].generation == (uint64_t)(frame / 3));
                    for (size_t i = record_of[set] + 1; i < at; ++i) CHECK(!(calls[i].fn == "hipEventRecord" && calls[i].handle == released[set].ev.e));
                }
                record_of[set] = calls.size();
                CHECK(released[set].record(main_stream) == hipSuccess && calls[record_of[set]].stream == main_stream);
            }
            size_t at = calls.size();
            for (StreamMark &m : released) m.forget();      // the streams were drained (a resize, another number of frames in flight)
            CHECK(calls.size() == at);
        }
        // the renderer's own order from a fresh handle: record the set left, advance, wait on the set entered
        StreamMark fresh[3];
        for (StreamMark &m : fresh) CHECK(m.create(hipEventDisableTiming) == hipSuccess);
        int cur = 0;
        for (int frame = 0; frame < 4; ++frame) {
            CHECK(fresh[cur].record(main_stream) == hipSuccess);
            cur = (cur + 1) % 3;
            size_t at = calls.size();
            CHECK(fresh[cur].wait(s.a) == hipSuccess && (frame < 2 ? calls.size() == at : waited(at, s.a, fresh[cur].ev)));
        }
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
}

void reader_table() {
    const char *name = "reader-table";
    char buf[6] = {};
    {
        TwoStreams s;
        ReaderTable<4> t;
        StreamMark *m = nullptr, *again = nullptr;
        CHECK(s.make());
        size_t at = calls.size();
        CHECK(t.ensure(hipEventDisableTiming) == hipSuccess && since(at) == "hipEventCreateWithFlags hipEventCreateWithFlags hipEventCreateWithFlags hipEventCreateWithFlags");
        CHECK(t.ensure(hipEventDisableTiming) == hipSuccess && calls.size() == at + 4);
        at = calls.size();
        CHECK(t.wait_for(&buf[0], s.a) == hipSuccess && t.wait_for(nullptr, s.a) == hipSuccess && calls.size() == at);   // nobody reads it: nothing
        CHECK(t.claim(&buf[0], s.b, m) == hipSuccess && m == &t.slot[0].done && m->record(s.b) == hipSuccess);
        CHECK(t.claim(&buf[1], s.b, m) == hipSuccess && m == &t.slot[1].done && m->record(s.b) == hipSuccess);
        CHECK(t.claim(&buf[0], s.b, again) == hipSuccess && again == &t.slot[0].done && again->record(s.b) == hipSuccess);   // the same buffer: its slot again
        CHECK(since(at) == "hipEventRecord hipEventRecord hipEventRecord" && t.slot[0].done.generation == 2 && !t.slot[2].ptr);
        at = calls.size();
        CHECK(t.wait_for(&buf[5], s.a) == hipSuccess && calls.size() == at);                                  // an unknown buffer: nothing
        CHECK(t.wait_for(&buf[0], s.a) == hipSuccess && waited(at, s.a, t.slot[0].done.ev) && !t.slot[0].ptr);   // a known one: one wait, and the slot is free
        CHECK(t.wait_for(&buf[0], s.a) == hipSuccess && calls.size() == at + 1);
        CHECK(t.claim(&buf[2], s.b, m) == hipSuccess && m == &t.slot[0].done);                                // the first free slot
        CHECK(t.claim(&buf[3], s.b, m) == hipSuccess && m == &t.slot[2].done && t.claim(&buf[4], s.b, m) == hipSuccess && m == &t.slot[3].done);
        CHECK(calls.size() == at + 1);                                                                        // (claiming alone calls nothing)
        at = calls.size();
        CHECK(t.claim(&buf[5], s.b, m) == hipSuccess && since(at) == "hipStreamSynchronize" && calls[at].handle == s.b.s);   // a fifth buffer: the readers' stream is drained, once
        CHECK(m == &t.slot[0].done && t.slot[0].ptr == &buf[5] && !t.slot[1].ptr && !t.slot[2].ptr && !t.slot[3].ptr);
        refuse_wait = 1;                                                                                      // a refused wait keeps the slot
        CHECK(m->record(s.b) == hipSuccess && t.wait_for(&buf[5], s.a) == hipErrorInvalidValue && t.slot[0].ptr == &buf[5]);
        ReaderTable<4> moved = std::move(t);
        CHECK(!t.slot[0].ptr && !t.slot[0].done.ev && !t.slot[0].done.recorded && moved.slot[0].ptr == &buf[5] && moved.slot[0].done.recorded);
        at = calls.size();
        CHECK(t.wait_for(&buf[5], s.a) == hipSuccess && calls.size() == at && moved.wait_for(&buf[5], s.a) == hipSuccess && waited(at, s.a, moved.slot[0].done.ev));
        at = calls.size();
        moved.release(); moved.release();
        CHECK(since(at) == "hipEventDestroy hipEventDestroy hipEventDestroy hipEventDestroy" && !moved.slot[0].ptr);
    }
    CHECK(alive() == 0 && double_releases == 0);
    done(name);
    name = "mark-moves-and-release";
    {
        TwoStreams s;
        StreamMark a, b;
        CHECK(s.make() && a.create(hipEventDisableTiming) == hipSuccess && b.create(hipEventDisableTiming) == hipSuccess && a.record(s.a) == hipSuccess);
        const hipEvent_t ev = a.ev;
        StreamMark c = std::move(a);
        CHECK(!a.ev && !a.recorded && a.on == nullptr && a.generation == 0 && c.ev == ev && c.recorded && c.on == s.a && c.generation == 1);
        size_t at = calls.size();
        CHECK(a.wait(s.b) == hipSuccess && calls.size() == at);     // a moved-from mark is empty: nothing to wait for
        b = std::move(c);                                            // move assignment releases what it held
        CHECK(since(at) == "hipEventDestroy" && live[EVENT].size() == 1 && b.ev == ev && b.recorded && !c.ev && !c.recorded);
        at = calls.size();
        CHECK(b.wait(s.b) == hipSuccess && waited(at, s.b, ev));
        at = calls.size();
        CHECK(b.create(hipEventDisableTiming) == hipSuccess && since(at) == "hipEventDestroy hipEventCreateWithFlags" && !b.recorded);   // made again: never recorded
        b.release(); b.release(); a.release();
        CHECK(since(at + 2) == "hipEventDestroy" && live[EVENT].empty());
    }
    CHECK(alive() == 0 && double_releases == 0);
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
    marks();
    ring_of_marks();
    reader_table();
    const char *name = "all-released-once";
    if (alive() != 0 || double_releases != 0) { std::printf("BAD %s: %zu handles alive, %d released twice\n", name, alive(), double_releases); ++failures; }
    else done(name);
    return failures ? 1 : 0;
}
