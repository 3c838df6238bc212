// device_resources.h -- owners of what the HIP runtime hands out: device memory, pinned memory, events, streams, the ring of pinned
// slots that host tables travel through, and the marks that order one stream behind another.  Host only, nothing of the project: every type is move-only and its destructor releases what it
// holds, so a handle (renderer_state.h) frees nothing by hand -- its members go in reverse order of declaration, a local owner on a failure path
// goes with its scope.  The owners make exactly the runtime calls the code they replace made; none of them synchronises behind the caller's
// back except Stream, whose release waits for the stream before it destroys it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace arctic {

// device memory.  ensure: room for `bytes`, with a quarter of headroom when it has to grow (what it held is gone then); alloc_exact: the true
// size, for what is allocated once
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        return alloc(bytes + bytes / 4 + 256);
    }
    hipError_t alloc_exact(size_t bytes) {
        release();
        return alloc(bytes);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    explicit operator bool() const { return p != nullptr; }
    template <class T> T *as() const { return static_cast<T *>(p); }

private:
    hipError_t alloc(size_t want) {
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
};

// pinned host memory (hipHostMalloc with the caller's flags); for mapped memory also the address the device writes it through
struct PinnedBuf {
    void *p = nullptr, *d = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), d(std::exchange(o.d, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); d = std::exchange(o.d, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    ~PinnedBuf() { release(); }
    hipError_t alloc(size_t bytes, unsigned flags) {   // (what it held is freed first)
        if (p) { hipError_t e = hipHostFree(p); p = d = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes;
        if ((flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) release();
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = d = nullptr; cap = 0; }
    explicit operator bool() const { return p != nullptr; }
    template <class T> T *as() const { return static_cast<T *>(p); }
    template <class T> T *dev() const { return static_cast<T *>(d); }
};

// an event: created explicitly (create) or where it is first needed (ensure), destroyed once
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = std::exchange(o.e, nullptr); } return *this; }
    ~Event() { release(); }
    hipError_t create(unsigned flags) { release(); return hipEventCreateWithFlags(&e, flags); }
    hipError_t ensure(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

// a stream the holder created; release waits for what it still holds, then destroys it
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s = std::exchange(o.s, nullptr); } return *this; }
    ~Stream() { release(); }
    hipError_t create(unsigned flags) { release(); return hipStreamCreateWithFlags(&s, flags); }
    void release() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } s = nullptr; }
    operator hipStream_t() const { return s; }
};

// Staged uploads: a table is written into a pinned slot and sent with ONE asynchronous copy; the slot is handed out again only after the copy
// that last read it has completed (its event), so with N slots an upload waits for the copy N uploads ago at most -- never for a kernel.
//   stage(capacity, &host)   waits for the current slot's copy if one is pending, makes the slot (or makes it again when it holds less than
//                            `capacity`), and gives its host address
//   send(dst, bytes, stream) copies the slot to `dst`, records the slot's event behind the copy, marks the slot pending and moves on to the
//                            next slot; bytes == 0: nothing to send, the ring moves on all the same
// Whether a table needs sending at all is the caller's business.
template <int N> struct UploadRing {
    struct Slot { PinnedBuf h; Event copied; bool pending = false; };
    Slot slot[N];
    int turn = 0;
    UploadRing() = default;
    UploadRing(UploadRing &&o) noexcept : turn(std::exchange(o.turn, 0)) { for (int k = 0; k < N; ++k) take(slot[k], o.slot[k]); }
    UploadRing &operator=(UploadRing &&o) noexcept {
        if (this != &o) { turn = std::exchange(o.turn, 0); for (int k = 0; k < N; ++k) take(slot[k], o.slot[k]); }
        return *this;
    }
    template <class T> hipError_t stage(size_t capacity_bytes, T **host) {
        Slot &s = slot[turn];
        hipError_t e;
        if (s.pending) { if ((e = hipEventSynchronize(s.copied)) != hipSuccess) return e; s.pending = false; }
        if (s.h.cap < capacity_bytes && (e = s.h.alloc(capacity_bytes, hipHostMallocDefault)) != hipSuccess) return e;
        if ((e = s.copied.ensure(hipEventDisableTiming)) != hipSuccess) return e;
        *host = s.h.template as<T>();
        return hipSuccess;
    }
    hipError_t send(void *dst, size_t bytes, hipStream_t stream) {
        Slot &s = slot[turn];
        turn = (turn + 1) % N;
        if (bytes == 0) return hipSuccess;
        hipError_t e;
        if ((e = hipMemcpyAsync(dst, s.h.p, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
        if ((e = hipEventRecord(s.copied, stream)) != hipSuccess) return e;
        s.pending = true;
        return hipSuccess;
    }
    void release() { for (Slot &s : slot) { s.h.release(); s.copied.release(); s.pending = false; } }   // (the turn stays; the caller has drained the stream)

private:
    static void take(Slot &a, Slot &b) { a.h = std::move(b.h); a.copied = std::move(b.copied); a.pending = std::exchange(b.pending, false); }
};

// A mark: one event that knows what it stands for -- whether anything has been recorded on it since it was made or forgotten, on which stream,
// and how many times.  The rules of cross-stream ordering are kept here, once, not at every site:
//   never recorded                          nothing to wait for
//   recorded on the waiting stream itself   nothing to wait for (stream order does it)
//   wait_once                               one wait per recording and waiter (`seen` is the waiter's: the generation it has waited for)
// `recorded` is apart from `on` because nullptr is a real stream, the default one.  forget: the caller has drained the streams, what was recorded
// is complete; the generation goes on counting, so no waiter's `seen` can match a later recording by accident.
struct StreamMark {
    Event ev;
    bool recorded = false;
    hipStream_t on = nullptr;
    uint64_t generation = 0;
    StreamMark() = default;
    StreamMark(StreamMark &&o) noexcept
        : ev(std::move(o.ev)), recorded(std::exchange(o.recorded, false)), on(std::exchange(o.on, nullptr)), generation(std::exchange(o.generation, 0)) {}
    StreamMark &operator=(StreamMark &&o) noexcept {
        if (this != &o) { ev = std::move(o.ev); recorded = std::exchange(o.recorded, false); on = std::exchange(o.on, nullptr); generation = std::exchange(o.generation, 0); }
        return *this;
    }
    hipError_t create(unsigned flags) { forget(); return ev.create(flags); }
    hipError_t ensure(unsigned flags) { return ev.ensure(flags); }
    void release() { ev.release(); forget(); }
    void forget() { recorded = false; on = nullptr; }
    hipError_t record(hipStream_t stream) {
        hipError_t e = hipEventRecord(ev, stream);
        if (e == hipSuccess) { recorded = true; on = stream; ++generation; }
        return e;
    }
    hipError_t wait(hipStream_t stream) const { return !recorded || stream == on ? hipSuccess : hipStreamWaitEvent(stream, ev, 0); }
    hipError_t wait_once(hipStream_t stream, uint64_t &seen) const {   // (a refused wait leaves `seen` as it was: the next call waits again)
        if (seen == generation) return hipSuccess;
        hipError_t e = wait(stream);
        if (e == hipSuccess) seen = generation;
        return e;
    }
};

// Who still reads this buffer: N slots of {buffer, mark recorded behind its reader}.
//   claim(ptr, drain, mark)  the slot that holds `ptr`, else a free one, else -- none free -- `drain` is waited for, every slot is cleared and slot 0
//                            taken; `mark` is the slot's, for the caller to record behind the reader it enqueues
//   wait_for(ptr, stream)    a slot holds `ptr`: `stream` waits for its mark and the slot is free again; else nothing
template <int N> struct ReaderTable {
    struct Slot { const void *ptr = nullptr; StreamMark done; };
    Slot slot[N];
    ReaderTable() = default;
    ReaderTable(ReaderTable &&o) noexcept { for (int k = 0; k < N; ++k) take(slot[k], o.slot[k]); }
    ReaderTable &operator=(ReaderTable &&o) noexcept { if (this != &o) for (int k = 0; k < N; ++k) take(slot[k], o.slot[k]); return *this; }
    hipError_t ensure(unsigned flags) {
        for (Slot &s : slot) { hipError_t e = s.done.ensure(flags); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    void release() { for (Slot &s : slot) { s.done.release(); s.ptr = nullptr; } }
    hipError_t wait_for(const void *ptr, hipStream_t stream) {
        for (Slot &s : slot)
            if (ptr && s.ptr == ptr) { hipError_t e = s.done.wait(stream); if (e != hipSuccess) return e; s.ptr = nullptr; }
        return hipSuccess;
    }
    hipError_t claim(const void *ptr, hipStream_t drain, StreamMark *&mark) {
        Slot *found = nullptr;
        for (Slot &s : slot) if (s.ptr == ptr) found = &s;
        if (!found) for (Slot &s : slot) if (!s.ptr) { found = &s; break; }
        if (!found) {
            hipError_t e = hipStreamSynchronize(drain);
            if (e != hipSuccess) return e;
            for (Slot &s : slot) s.ptr = nullptr;
            found = &slot[0];
        }
        found->ptr = ptr;
        mark = &found->done;
        return hipSuccess;
    }

private:
    static void take(Slot &a, Slot &b) { a.ptr = std::exchange(b.ptr, nullptr); a.done = std::move(b.done); }
};

}  // namespace arctic
