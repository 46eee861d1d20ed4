// agx_resources.h - HOST side: where a handle of this library gets its storage from.  Two small things:
//   BlockLayout     "one device block carved into 256-byte-aligned sections": add() the sections in order, ask for bytes()
//   ResourcesT<Api> the owner of a handle's device memory, pinned host memory, events and streams: every acquisition is
//                   recorded, release() (and the destructor) gives everything back exactly once, on the owner's device
// so that a create which fails at its N-th call, and every destroy, is "delete the handle".  The runtime comes through a
// policy class (agx_api.hip has the HIP one, the only place in csrc/ that names the runtime's allocation calls) so that
// tests/resources_harness.cpp can drive the logic with a mocked runtime and fail any call of a sequence.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "agx_device_guard.h"

namespace agx {

struct BlockLayout {
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    // the offset of a new section of `b` bytes behind those added so far (a zero-byte section takes no space)
    size_t add(size_t b) {
        const size_t at = total;
        total += pad(b);
        return at;
    }
    size_t bytes() const { return total; }
    template <class T>
    static T *at(uint8_t *block, size_t offset) { return reinterpret_cast<T *>(block + offset); }

private:
    size_t total = 0;
};

// Api: DeviceGuardT's get / set, an Error type whose value-initialised value means success, and
//   Error device_alloc(void **, size_t)  void device_free(void *)     Error pinned_alloc(void **, size_t)  void pinned_free(void *)
//   Error event_create(void **, unsigned flags)                       void event_destroy(void *)
//   Error stream_create(void **, unsigned flags)  Error stream_create_priority(void **, unsigned flags, int)  void stream_destroy(void *)
template <class Api>
class ResourcesT {
public:
    using Error = typename Api::Error;
    const int device;        // the ordinal everything here lives on: release() needs no other live object to find it

    explicit ResourcesT(int dev) : device(dev) {}
    ~ResourcesT() { release(); }
    ResourcesT(const ResourcesT &) = delete;
    ResourcesT &operator=(const ResourcesT &) = delete;

    // Each returns the runtime's own error code (the caller words the message); a failed call records nothing and leaves *out alone.
    template <class T>
    Error device_mem(T **out, size_t bytes) {
        return take(kDevice, out, [&](void **p) { return Api::device_alloc(p, bytes); });
    }
    template <class T>
    Error pinned(T **out, size_t bytes) {
        return take(kPinned, out, [&](void **p) { return Api::pinned_alloc(p, bytes); });
    }
    template <class E>
    Error event(E *out, unsigned flags) {
        return take(kEvent, out, [&](void **p) { return Api::event_create(p, flags); });
    }
    template <class S>
    Error stream(S *out, unsigned flags) {
        return take(kStream, out, [&](void **p) { return Api::stream_create(p, flags); });
    }
    template <class S>
    Error stream(S *out, unsigned flags, int priority) {
        return take(kStream, out, [&](void **p) { return Api::stream_create_priority(p, flags, priority); });
    }

    // Everything recorded goes back, latest first, with `device` current (the caller's device is put back afterwards); the
    // owner is empty then and can be used again.
    void release() {
        if (items.empty()) return;
        DeviceGuardT<Api> g(device);
        for (size_t i = items.size(); i-- > 0;) {
            void *h = items[i].handle;
            switch (items[i].kind) {
                case kDevice: Api::device_free(h); break;
                case kPinned: Api::pinned_free(h); break;
                case kEvent: Api::event_destroy(h); break;
                case kStream: Api::stream_destroy(h); break;
            }
        }
        items.clear();
    }

private:
    enum Kind : uint8_t { kDevice, kPinned, kEvent, kStream };
    struct Item {
        Kind kind;
        void *handle;
    };
    std::vector<Item> items;

    template <class P, class Make>
    Error take(Kind kind, P *out, Make &&make) {
        items.reserve(items.size() + 1);        // (so that recording cannot fail once the runtime has handed something out)
        void *h = nullptr;
        const Error e = make(&h);
        if (e != Error()) return e;
        if (h) items.push_back(Item{kind, h});  // (a zero-byte allocation is a null pointer: nothing to give back)
        *out = static_cast<P>(h);
        return e;
    }
};

}  // namespace agx
