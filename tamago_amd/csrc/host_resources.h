// Move-only owners of the HIP resources of a host-side handle (tg_search, tg_selfplay: csrc/search.hip; tg_net: csrc/net_device.h).
// Host code only.
//
// A resource that is a member of a handle is released exactly once, by the handle's destructor - which the destroy function of a
// search handle runs after it has synchronised the handle's launch stream, so nothing queued there still uses it (a network
// has no stream of its own: hipFree waits for the device).  Every call returns a TG_* code;
// a HIP failure goes through tg::fail with the HIP error string (TG_HIP).  No owner synchronises anything on its own except
// where its comment says so: what has to be idle before a buffer is released early is the business of the site that does it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "common.h"

namespace tg {

// A hipMalloc allocation and its capacity in elements.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    void reset() {                                   // (hipFree synchronises the device implicitly)
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // at least `count` elements; grown by free-then-allocate: the contents are NOT kept
    int reserve(size_t count) {
        if (count <= cap_) return TG_OK;
        reset();
        TG_HIP(hipMalloc(reinterpret_cast<void **>(&p_), count * sizeof(T)));
        cap_ = count;
        return TG_OK;
    }
    int alloc_zeroed(size_t count) {
        if (int rc = reserve(count)) return rc;
        // hipMemset on device memory is asynchronous (legacy null stream); callers go on to use the
        // buffer from NON-BLOCKING streams (torch side streams), which the null stream does not order
        TG_HIP(hipMemset(p_, 0, count * sizeof(T)));
        TG_HIP(hipStreamSynchronize(nullptr));
        return TG_OK;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// A hipHostMalloc allocation (flags: hipHostMallocDefault or hipHostMallocMapped) and, for mapped memory, its device address.
template <typename T>
class PinBuf {
public:
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { reset(); }

    T *get() const { return p_; }
    T *dev() const { return dev_; }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = dev_ = nullptr;
    }
    int alloc(size_t count, unsigned flags = hipHostMallocDefault) {      // (an earlier allocation is released; contents not kept)
        reset();
        T *p = nullptr, *d = nullptr;
        TG_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), flags));
        if (flags & hipHostMallocMapped) {
            const hipError_t e = hipHostGetDevicePointer(reinterpret_cast<void **>(&d), p, 0);
            if (e != hipSuccess) {
                (void)hipHostFree(p);
                return tg::fail(TG_ERR_HIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e));
            }
        }
        p_ = p;
        dev_ = d;
        return TG_OK;
    }

private:
    T *p_ = nullptr, *dev_ = nullptr;
};

// An event without timing, created at its first use, and whether it has ever been recorded.
class Event {
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e_) (void)hipEventDestroy(e_); }

    hipEvent_t get() const { return e_; }
    bool recorded() const { return recorded_; }
    int create() {
        if (!e_) TG_HIP(hipEventCreateWithFlags(&e_, hipEventDisableTiming));
        return TG_OK;
    }
    int record(hipStream_t st) {
        if (int rc = create()) return rc;
        TG_HIP(hipEventRecord(e_, st));
        recorded_ = true;
        return TG_OK;
    }
    int wait_if_recorded() {                          // the HOST waits
        if (recorded_) TG_HIP(hipEventSynchronize(e_));
        return TG_OK;
    }

private:
    hipEvent_t e_ = nullptr;
    bool recorded_ = false;
};

// A non-blocking stream, created on request; the destructor waits for what is queued on it.
class Stream {
public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        if (!s_) return;
        (void)hipStreamSynchronize(s_);
        (void)hipStreamDestroy(s_);
    }

    hipStream_t get() const { return s_; }
    int create() {
        if (!s_) TG_HIP(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        return TG_OK;
    }

private:
    hipStream_t s_ = nullptr;
};

// Pinned staging for a small upload that is repeated call after call: N slots of `per_slot` elements, used in turn, each
// with the event behind the last copy out of it.  The host fills the slot and queues the copy without waiting for the
// stream; it only waits - practically never - for the copy N calls ago.
//   T *pin; int slot;
//   if (int rc = ring.acquire(n, &pin, &slot)) return rc;        // first use: allocates; waits for the slot's last copy
//   ... fill pin[0 .. n) ...
//   hipMemcpyAsync(dst, pin, ..., stream);  (or a kernel that reads ring.dev(slot): mapped memory)
//   ring.commit(slot, stream);
// A slot that was acquired and never committed is harmless: its event stays as it was.
template <typename T, int N>
class StagingRing {
public:
    int acquire(size_t per_slot, T **ptr, int *slot, unsigned flags = hipHostMallocDefault) {
        if (!pin_.get()) {
            if (int rc = pin_.alloc((size_t)N * per_slot, flags)) return rc;
            per_slot_ = per_slot;
        }
        const int i = (int)(seq_++ % N);
        if (int rc = ev_[i].wait_if_recorded()) return rc;
        *ptr = pin_.get() + (size_t)i * per_slot_;
        *slot = i;
        return TG_OK;
    }
    int commit(int slot, hipStream_t st) { return ev_[slot].record(st); }
    T *dev(int slot) const { return pin_.dev() + (size_t)slot * per_slot_; }     // (hipHostMallocMapped rings)

private:
    PinBuf<T> pin_;
    Event ev_[N];
    size_t per_slot_ = 0;
    unsigned seq_ = 0;
};

}  // namespace tg
