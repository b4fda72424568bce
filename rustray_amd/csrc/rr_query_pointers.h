// rr_query_pointers.h — may the kernels of a scene's device read or write a buffer the caller handed to a device-buffer ray query
// (rr_trace_rays_device, rr_trace_shadow_rays_device, rr_shade_rays_device)?  Plain host logic, no HIP calls: rr_api_query.h classifies the
// pointer (hipPointerGetAttributes) and looks up the peer state, this header decides; tests/native/query_pointer_test.cpp checks the
// whole table on the CPU.  A pointer that fails here never reaches a launch: the call returns RR_ERR_INVALID_ARGUMENT naming the argument.
#pragma once

// what the runtime says a pointer is
enum QueryMemKind {
    RR_QMEM_UNREGISTERED = 0, // pageable host memory the runtime has never seen (malloc, a numpy array), or not a valid pointer at all
    RR_QMEM_HOST = 1,         // pinned or registered host memory (hipHostMalloc, hipHostRegister): mapped into every device
    RR_QMEM_DEVICE = 2,       // device memory (hipMalloc, a torch tensor) of `owner_device`
    RR_QMEM_MANAGED = 3,      // hipMallocManaged: migrates or is mapped, addressable by every device
    RR_QMEM_ARRAY = 4,        // a hipArray: opaque layout, not a linear buffer
    RR_QMEM_KINDS = 5
};

// owner_device: the device that holds the allocation (RR_QMEM_DEVICE only); peer_enabled: scene_device has peer access to owner_device
// ENABLED (hipDeviceEnablePeerAccess has succeeded in this process; that the link exists is not enough).
inline bool query_pointer_ok(QueryMemKind kind, int owner_device, int scene_device, bool peer_enabled) {
    switch (kind) {
    case RR_QMEM_HOST:
    case RR_QMEM_MANAGED:
        return true;
    case RR_QMEM_DEVICE:
        if (owner_device < 0 || scene_device < 0) return false;
        return owner_device == scene_device || peer_enabled;
    case RR_QMEM_UNREGISTERED:
    case RR_QMEM_ARRAY:
    default:
        return false;
    }
}

inline const char* query_mem_kind_name(QueryMemKind kind) {
    switch (kind) {
    case RR_QMEM_UNREGISTERED: return "unregistered host memory";
    case RR_QMEM_HOST: return "pinned host memory";
    case RR_QMEM_DEVICE: return "device memory";
    case RR_QMEM_MANAGED: return "managed memory";
    case RR_QMEM_ARRAY: return "a hipArray";
    default: return "memory of an unknown kind";
    }
}
