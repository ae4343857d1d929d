// Ownership of everything an opaque handle (ch_model, ch_trainer, ch_text) holds on the device: memory blocks, pinned host
// blocks, streams and events.  A handle embeds ONE owner, takes every resource from it and never frees anything itself:
// `delete handle` destroys events, then streams, then memory.  ChDeviceTemp is the scoped form for a staging buffer that
// lives for one function call.
//
// Both are templates over the backend `Api` (static functions, resolved at compile time: the product instantiation below
// calls HIP directly).  The seam exists so that tests/device_owner_test.cpp can compile this very header on the CPU against a
// backend that counts live objects and fails the k-th call -- an allocation failure cannot be provoked on a GPU.
#pragma once
#include <stddef.h>

#include <string>
#include <vector>

#include "ch_host.h"

template <class Api>
class ChDeviceOwnerT {
   public:
    using stream_t = typename Api::stream_t;
    using event_t = typename Api::event_t;

    ChDeviceOwnerT() = default;
    ChDeviceOwnerT(const ChDeviceOwnerT &) = delete;
    ChDeviceOwnerT &operator=(const ChDeviceOwnerT &) = delete;
    ~ChDeviceOwnerT() {
        for (event_t e : events_) Api::event_destroy(e);
        for (stream_t s : streams_) Api::stream_destroy(s);
        for (void *p : host_) Api::host_free(p);
        for (const Block &b : blocks_) Api::free(b.p);
    }

    // One device allocation per call (a 0-byte request allocates and counts 16 bytes), optionally zero-filled.  nullptr + the
    // error string on failure; a block whose zero-fill failed stays owned (freed at destruction) but is not counted.
    void *alloc(size_t bytes, bool zero = false) {
        if (bytes == 0) bytes = 16;
        blocks_.push_back(Block{nullptr, 0});   // the slot first: nothing below can fail between the allocation and its registration
        void *p = Api::malloc(bytes);
        if (!p) {
            blocks_.pop_back();
            ch_set_error("hipMalloc failed for " + std::to_string(bytes) + " bytes");
            return nullptr;
        }
        blocks_.back().p = p;
        if (zero && !Api::memset_zero(p, bytes)) {
            ch_set_error("hipMemset failed for " + std::to_string(bytes) + " bytes");
            return nullptr;
        }
        blocks_.back().bytes = bytes;
        bytes_ += bytes;
        return p;
    }
    // Gives one owned block back and subtracts its size.  A pointer this owner does not hold is an error: nothing is freed.
    int release(void *p) {
        for (size_t i = 0; p && i < blocks_.size(); ++i)
            if (blocks_[i].p == p) {
                bytes_ -= blocks_[i].bytes;
                blocks_.erase(blocks_.begin() + i);
                if (Api::free(p)) return 0;
                ch_set_error("hipFree failed");
                return 1;
            }
        ch_set_error("release: the pointer is not a block of this handle");
        return 1;
    }
    // Release-then-alloc for a buffer that has to grow: *buf / *have name an owned block and its size, or nullptr / 0.
    // On any failure the caller is left with nullptr / 0, never with a freed pointer or a stale size.
    int regrow(void **buf, size_t *have, size_t need) {
        void *old = *buf;
        *buf = nullptr;
        *have = 0;
        if (old && release(old)) return 1;
        if (!(*buf = alloc(need))) return 1;
        *have = need;
        return 0;
    }
    size_t bytes() const { return bytes_; }

    void *host_alloc(size_t bytes) {   // pinned host memory (not part of bytes())
        host_.push_back(nullptr);
        void *p = Api::host_malloc(bytes);
        if (!p) {
            host_.pop_back();
            ch_set_error("hipHostMalloc failed for " + std::to_string(bytes) + " bytes");
            return nullptr;
        }
        return host_.back() = p;
    }
    stream_t stream(unsigned flags) {
        streams_.push_back(stream_t());
        stream_t s = Api::stream_create(flags);
        if (!s) {
            streams_.pop_back();
            ch_set_error("cannot create a stream");
            return stream_t();
        }
        return streams_.back() = s;
    }
    event_t event(unsigned flags = 0) {
        events_.push_back(event_t());
        event_t e = Api::event_create(flags);
        if (!e) {
            events_.pop_back();
            ch_set_error("cannot create an event");
            return event_t();
        }
        return events_.back() = e;
    }

   private:
    struct Block {
        void *p;
        size_t bytes;   // what bytes() counts for it
    };
    std::vector<Block> blocks_;
    std::vector<void *> host_;
    std::vector<stream_t> streams_;
    std::vector<event_t> events_;
    size_t bytes_ = 0;
};

// A device buffer that is freed when the scope ends, whichever way it ends.
template <class Api>
class ChDeviceTempT {
   public:
    ChDeviceTempT() = default;
    ChDeviceTempT(const ChDeviceTempT &) = delete;
    ChDeviceTempT &operator=(const ChDeviceTempT &) = delete;
    ~ChDeviceTempT() {
        if (p_) Api::free(p_);
    }
    int get(size_t bytes) {   // once per object; 1 + the error string on failure
        p_ = Api::malloc(bytes);
        if (p_ || bytes == 0) return 0;
        ch_set_error("hipMalloc failed for " + std::to_string(bytes) + " bytes (temporary)");
        return 1;
    }
    template <class T>
    T *as() const {
        return (T *)p_;
    }

   private:
    void *p_ = nullptr;
};

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
struct ChHipApi {
    using stream_t = hipStream_t;
    using event_t = hipEvent_t;
    static void *malloc(size_t bytes) {
        void *p = nullptr;
        return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
    }
    static bool free(void *p) { return hipFree(p) == hipSuccess; }
    static bool memset_zero(void *p, size_t bytes) { return hipMemset(p, 0, bytes) == hipSuccess; }
    static void *host_malloc(size_t bytes) {
        void *p = nullptr;
        return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    static void host_free(void *p) { (void)hipHostFree(p); }
    static stream_t stream_create(unsigned flags) {
        stream_t s = nullptr;
        return hipStreamCreateWithFlags(&s, flags) == hipSuccess ? s : nullptr;
    }
    static void stream_destroy(stream_t s) { (void)hipStreamDestroy(s); }
    static event_t event_create(unsigned flags) {
        event_t e = nullptr;
        return hipEventCreateWithFlags(&e, flags) == hipSuccess ? e : nullptr;
    }
    static void event_destroy(event_t e) { (void)hipEventDestroy(e); }
};
using ChDeviceOwner = ChDeviceOwnerT<ChHipApi>;
using ChDeviceTemp = ChDeviceTempT<ChHipApi>;
#endif
