// nbody_device_owned.h -- what a handle of the library owns on the device, as members that free themselves: DeviceArray<T>, and
// move-only owners of an event, a stream and an instantiated graph.  The context of a single system (nbody_ctx.h) and the handle
// of a batched ensemble (nbody_batch_handle.h) hold nothing else that HIP allocates, so deleting either frees all of it and
// no list of frees is kept by hand.  Internal: nothing here crosses the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

// Internal to the library: the names below are not exported, so its dynamic symbols stay those of the C ABI.
#pragma GCC visibility push(hidden)

namespace nbody {

// A device array of T that its owner frees: a pointer and the elements it has room for.
template <class T>
struct DeviceArray {
    T *ptr = nullptr;
    size_t capacity = 0;

    DeviceArray() = default;
    DeviceArray(DeviceArray &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), capacity(std::exchange(o.capacity, 0)) {}
    DeviceArray &operator=(DeviceArray &&o) noexcept  // the array held before goes with `o`
    {
        std::swap(ptr, o.ptr);
        std::swap(capacity, o.capacity);
        return *this;
    }
    ~DeviceArray() { release(); }

    // Room for `count` elements: nothing to do while the capacity suffices (0, an output the call was not asked for: always;
    // a size fixed per handle: after the first call that asked); otherwise a new array in place of the old one, whose contents
    // no call needs (gravity's rows grow with the call).  A failed allocation leaves no array.
    hipError_t ensure(size_t count)
    {
        if (count <= capacity)
            return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void **)&ptr, sizeof(T) * count);
        if (e == hipSuccess)
            capacity = count;
        return e;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        capacity = 0;
    }
};

// The three owners below hold one HIP handle each, or none; they convert to it, so a HIP call takes the member as it took the
// raw handle, and the creating call writes `.h`.  Moving leaves the source empty (a move assignment hands it the old handle).
struct OwnedEvent {
    hipEvent_t h = nullptr;
    OwnedEvent() = default;
    OwnedEvent(OwnedEvent &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    OwnedEvent &operator=(OwnedEvent &&o) noexcept { std::swap(h, o.h); return *this; }
    ~OwnedEvent() { if (h) (void)hipEventDestroy(h); }
    operator hipEvent_t() const { return h; }
};

struct OwnedStream {
    hipStream_t h = nullptr;
    OwnedStream() = default;
    OwnedStream(OwnedStream &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    OwnedStream &operator=(OwnedStream &&o) noexcept { std::swap(h, o.h); return *this; }
    ~OwnedStream() { if (h) (void)hipStreamDestroy(h); }
    operator hipStream_t() const { return h; }
};

struct OwnedGraphExec {
    hipGraphExec_t h = nullptr;
    OwnedGraphExec() = default;
    OwnedGraphExec(OwnedGraphExec &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    OwnedGraphExec &operator=(OwnedGraphExec &&o) noexcept { std::swap(h, o.h); return *this; }
    ~OwnedGraphExec() { reset(); }
    void reset() { if (h) (void)hipGraphExecDestroy(h); h = nullptr; }
    operator hipGraphExec_t() const { return h; }
};

}  // namespace nbody

#pragma GCC visibility pop
