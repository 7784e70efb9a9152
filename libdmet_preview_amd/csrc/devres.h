// Scoped owners of device resources (host code only): a device allocation, a stream, an event, and the double-buffered host feed
// built from them.  Move-only, no policy beyond "released when it goes out of scope".  DESTRUCTORS DO NOT SYNCHRONISE: whoever
// lets an owner go while work that uses it may still be in flight synchronises the stream first, at the call site -- or declares a
// StreamDrain after the owners.  Carver cuts one allocation into arrays.
#pragma once
#include "common.h"
#include <algorithm>
#include <utility>

class DevMem {
    void *p_ = nullptr;
    size_t n_ = 0;
public:
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevMem &operator=(DevMem &&o) noexcept {        // (what was held is freed here, not when `o` goes)
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
    ~DevMem() { reset(); }
    // a fresh block of `bytes` in place of what was held (through dmk_dev_alloc: the out-of-memory hook gets its turn); on
    // failure the owner is empty and the error is returned
    hipError_t alloc(dmk_ctx *ctx, size_t bytes) {
        reset();
        const hipError_t e = dmk_dev_alloc(ctx, &p_, bytes);
        if (e == hipSuccess) n_ = bytes; else p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    // the boundary to raw pointers (the workspaces parked in the context): take over / give up a block without freeing it
    void adopt(void *p, size_t bytes) { reset(); p_ = p; n_ = p ? bytes : 0; }
    void *release() { void *p = p_; p_ = nullptr; n_ = 0; return p; }
    template <class T> T *get() const { return static_cast<T *>(p_); }
    size_t bytes() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// carves 256-byte aligned arrays of doubles out of one allocation (first pass over a null base: the size)
struct Carver {
    char *p;
    explicit Carver(void *base) : p(static_cast<char *>(base)) {}
    double *take(long long count) { double *q = reinterpret_cast<double *>(p); p += dmk_align256((size_t)std::max<long long>(count, 1) * 8); return q; }
};

// drains a stream when it goes out of scope.  Declared AFTER the owners of the device memory that the queued work uses: destructors
// run in reverse order, so the stream is drained before they let go
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// a stream or an event: what DevStream and DevEvent share
template <class H, hipError_t (*Destroy)(H)> class DevHandle {
protected:
    H h_ = nullptr;
public:
    DevHandle() = default;
    DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevHandle &operator=(DevHandle &&o) noexcept { std::swap(h_, o.h_); return *this; }
    ~DevHandle() { if (h_) (void)Destroy(h_); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
};
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {       // non-blocking
    hipError_t create() { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
};
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {          // without timing
    hipError_t create() { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, hipEventDisableTiming); }
};

// THE HOST FEED: blocks in host memory are uploaded on a copy stream into one of two device staging blocks while the compute
// stream (ctx->stream) works on the other.  Per slot: `copied` -- the upload has landed (recorded on the copy stream, the compute
// stream waits on it), `consumed` -- the kernels that read the staging block have run (recorded on the compute stream by done(),
// the next upload into the slot waits on it; recorded once at open, so the first upload waits on nothing).  A slot's staging block
// is allocated on its first use.  The feed is whole or absent: open() builds all of it or none.
class HostFeed {
    dmk_ctx *ctx_ = nullptr;
    DevStream copy_;
    DevEvent copied_[2], consumed_[2];
    DevMem stage_[2];
public:
    bool is_open() const { return (bool)copy_; }
    int open(dmk_ctx *ctx) {
        if (is_open()) return DMK_OK;
        DevStream s;
        DevEvent ev[4];
        DMK_HIP(ctx, s.create());
        for (DevEvent &e : ev) DMK_HIP(ctx, e.create());
        for (int i = 0; i < 2; ++i) DMK_HIP(ctx, hipEventRecord(ev[2 + i].get(), ctx->stream));
        ctx_ = ctx;
        copy_ = std::move(s);
        for (int i = 0; i < 2; ++i) { copied_[i] = std::move(ev[i]); consumed_[i] = std::move(ev[2 + i]); }
        return DMK_OK;
    }
    // `bytes` from host memory into the staging block of `slot`; the compute stream is made to wait for them.  *dev: the block.
    int stage(int slot, const void *host, size_t bytes, void **dev) {
        if (!stage_[slot] && stage_[slot].alloc(ctx_, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return dmk_fail(ctx_, DMK_ERR_NOMEM, "host feed: no memory for a staging block (%zu bytes)", bytes);
        }
        if (bytes > stage_[slot].bytes()) return dmk_fail(ctx_, DMK_ERR_INVALID, "host feed: block larger than the staging block");
        DMK_HIP(ctx_, hipStreamWaitEvent(copy_.get(), consumed_[slot].get(), 0));
        DMK_HIP(ctx_, hipMemcpyAsync(stage_[slot].get<void>(), host, bytes, hipMemcpyHostToDevice, copy_.get()));
        DMK_HIP(ctx_, hipEventRecord(copied_[slot].get(), copy_.get()));
        DMK_HIP(ctx_, hipStreamWaitEvent(ctx_->stream, copied_[slot].get(), 0));
        *dev = stage_[slot].get<void>();
        return DMK_OK;
    }
    // everything enqueued on the compute stream so far is all that reads the staging block of `slot`
    int done(int slot) { DMK_HIP(ctx_, hipEventRecord(consumed_[slot].get(), ctx_->stream)); return DMK_OK; }
    // blocks the host until the last upload into `slot` has landed: its host buffer may be rewritten
    int wait_copied(int slot) { if (is_open()) DMK_HIP(ctx_, hipEventSynchronize(copied_[slot].get())); return DMK_OK; }
    void sync() { if (is_open()) (void)hipStreamSynchronize(copy_.get()); }
};
