// mld_batch_object.h — the host side the batch objects on top of the public C-ABI have in common (mld_tracks, mld_labels,
// mld_semantic_planes, mld_ransac_planes, mld_projected_clouds, mld_depth_reports, mld_plane_inliers, mld_feature_traces;
// each a translation unit of its own that includes this header, include/mld.h and - for what their kernels share -
// mld_batch_device.h only):
//   Object         the fields every object has (context, stream, device, last error), fail() and the MLD_HIP check on them
//   DeviceBuffer<T>  one allocation of device (or pinned host) memory, returned by its destructor: the only place of
//                  the batch objects that takes or returns GPU memory
//   DescRing<D>    the per-call table of n_seq descriptors: staged on the host, copied into one of kGens pinned
//                  generations and moved to device memory by a kernel on the object's stream
//   CompactScratch the device scratch of a pass / scan / write stream compaction (mld_batch_device.h) and its sizes
//   create_object / release_object / destroy_object   the skeleton of mld_*_create and mld_*_destroy
//   no_object, misaligned, with_stride   the refusal of a call on no object, the alignment test, the 16 / 32 dispatch
// Who frees what: an object's members own its memory (buffers, ring, scratch), so `delete` returns all of it and a unit
// has nothing to free by hand.  release_object deletes after the stream has been synchronised, with the object's
// device current; objects live on the heap only (create_object / release_object), so no destructor runs at exit.
// The objects share these TYPES; every object has its own ring, and none of this is shared with the context's own
// upload ring in mld_api.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../include/mld.h"

namespace mld_batch {

constexpr int kGens = 16;  // pinned generations of a descriptor table: the host may run this many uploads ahead

namespace {  // (internal linkage: every translation unit that includes this header gets its own kernel and host stub)

__global__ __launch_bounds__(256) void k_batch_upload(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src_host,
                                                      int n_words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) dst[i] = __builtin_nontemporal_load(src_host + i);
}

}  // namespace

struct Object {
    mld_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;  // the context's
    int device = 0;                // that stream's
    std::string err;               // mld_*_last_error(object)
};

inline int fail(Object* o, int code, const char* text) {
    o->err = text;
    return code;
}

// A call on no object: "<fn>: null object (<arg>)" into the unit's text for mld_*_last_error(NULL).
inline int no_object(char (&no_object_error)[512], const char* fn, const char* arg) {
    std::snprintf(no_object_error, sizeof(no_object_error), "%s: null object (%s)", fn, arg);
    return MLD_ERR_INVALID_ARG;
}

inline bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// f(std::integral_constant<int, 16 or 32>) for the stride of a cloud record (anything else was refused before).
template <typename F>
void with_stride(int stride_bytes, F f) {
    if (stride_bytes == 16)
        f(std::integral_constant<int, 16>{});
    else
        f(std::integral_constant<int, 32>{});
}

#define MLD_HIP(o, expr)                                                                                   \
    do {                                                                                                   \
        const hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                            \
            (o)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                  \
            return MLD_ERR_HIP;                                                                            \
        }                                                                                                  \
    } while (0)

// One allocation of `count` T that is returned when its owner goes: device memory, or (Pinned) page-locked host memory.
// Move-only, starts null, never grows.
template <typename T, bool Pinned = false>
class DeviceBuffer {
    T* p_ = nullptr;

public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& b) noexcept : p_(b.p_) { b.p_ = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&&) = delete;
    ~DeviceBuffer() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    }

    int allocate(Object* o, size_t count) {
        if (Pinned)
            MLD_HIP(o, hipHostMalloc((void**)&p_, count * sizeof(T), hipHostMallocDefault));
        else
            MLD_HIP(o, hipMalloc((void**)&p_, count * sizeof(T)));
        return MLD_OK;
    }

    T* get() const { return p_; }
};

template <typename Desc>
struct DescRing {
    static_assert(sizeof(Desc) % 4 == 0, "the upload kernel moves 32-bit words");
    DeviceBuffer<Desc> d_desc;                  // what the kernels of a call read
    DeviceBuffer<unsigned char, true> up_base;  // pinned: kGens generations of n_seq descriptors
    size_t gen_bytes = 0;
    hipEvent_t up_ev[kGens] = {};               // recorded behind the upload kernel that reads the generation
    bool up_busy[kGens] = {};
    int up_next = 0;
    std::vector<Desc> stage;                    // the next call's descriptors, filled by the caller

    DescRing() = default;
    DescRing(const DescRing&) = delete;
    // After the stream has been synchronised (release_object): the events first, then the two buffers.
    ~DescRing() {
        for (int g = 0; g < kGens; g++)
            if (up_ev[g]) (void)hipEventDestroy(up_ev[g]);
    }

    int allocate(Object* o, int n_seq) {
        stage.assign((size_t)n_seq, Desc{});
        gen_bytes = (size_t)n_seq * sizeof(Desc);
        int rc;
        if ((rc = d_desc.allocate(o, (size_t)n_seq))) return rc;
        if ((rc = up_base.allocate(o, gen_bytes * kGens))) return rc;
        for (int g = 0; g < kGens; g++) MLD_HIP(o, hipEventCreateWithFlags(&up_ev[g], hipEventDisableTiming));
        return MLD_OK;
    }

    // The staged descriptors to the device on the object's stream; `stage` may be rewritten as soon as this returns.
    int upload(Object* o) {
        const int g = up_next;
        if (up_busy[g]) MLD_HIP(o, hipEventSynchronize(up_ev[g]));  // (only when kGens uploads are still queued)
        unsigned char* pinned = up_base.get() + (size_t)g * gen_bytes;
        std::memcpy(pinned, stage.data(), gen_bytes);
        const int words = (int)(gen_bytes / 4);
        hipLaunchKernelGGL(k_batch_upload, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, o->stream,
                           reinterpret_cast<uint32_t*>(d_desc.get()), reinterpret_cast<const uint32_t*>(pinned), words);
        MLD_HIP(o, hipGetLastError());
        MLD_HIP(o, hipEventRecord(up_ev[g], o->stream));
        up_busy[g] = true;
        up_next = (g + 1) % kGens;
        return MLD_OK;
    }
};

// The device scratch of a stream compaction over sequences of up to max_items items: one 64-bit mask per group of 64
// items, and per chunk of `chunk` items (+ 1: the total) `columns` counts side by side.
struct CompactScratch {
    DeviceBuffer<unsigned long long> d_gm;
    DeviceBuffer<int> d_cpre;
    long long groups_per_seq = 0;
    long long chunks_per_seq = 0;

    int allocate(Object* o, int n_seq, int64_t max_items, int chunk, int columns, bool masks = true) {
        groups_per_seq = (long long)((max_items + 63) / 64);
        chunks_per_seq = (long long)((max_items + chunk - 1) / chunk);
        int rc;
        if (masks && (rc = d_gm.allocate(o, (size_t)n_seq * (size_t)groups_per_seq))) return rc;
        return d_cpre.allocate(o, (size_t)n_seq * (size_t)(chunks_per_seq + 1) * (size_t)columns);
    }
};

// Obj: an Object whose members own what it allocated (DeviceBuffer, DescRing, CompactScratch): delete returns all of it,
// with the object's device current and nothing of the object in flight.
template <typename Obj>
void release_object(Obj* o) {
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    delete o;
}

template <typename Obj>
void destroy_object(Obj* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    release_object(o);
}

// mld_*_create behind the argument checks, which hand in at most one verdict on the arguments, in the caller's own order
// (the sizes first, then the context, then the rest; or the context last): `refusal`, a whole text refused with
// MLD_ERR_INVALID_ARG (null: none), or `code` and `why`, refused with that code as "<fn>: <why>" (MLD_OK: none).
// `no_object_error` is the caller's string for mld_*_last_error(NULL).  init(obj) fills in the object's own fields and
// allocates, the ring included, on the stream's device.  Objects live on the heap only.
template <typename Obj, typename Init>
Obj* create_object(char (&no_object_error)[512], const char* fn, const char* refusal, mld_ctx* ctx, int* status_out, Init init,
                   int code = MLD_OK, const char* why = "") {
    auto refuse = [&](int status, const char* prefix, const char* text) -> Obj* {
        std::snprintf(no_object_error, sizeof(no_object_error), "%s%s", prefix, text);
        if (status_out) *status_out = status;
        return nullptr;
    };
    if (status_out) *status_out = MLD_OK;
    if (refusal) return refuse(MLD_ERR_INVALID_ARG, "", refusal);
    if (code != MLD_OK) return refuse(code, fn, (std::string(": ") + why).c_str());
    Obj* o = new (std::nothrow) Obj();
    if (!o) return refuse(MLD_ERR_HIP, fn, ": out of host memory");
    o->ctx = ctx;
    // the object lives on the context's stream and on that stream's device
    o->stream = static_cast<hipStream_t>(mld_get_stream(ctx));
    hipDevice_t dev = 0;
    if (hipStreamGetDevice(o->stream, &dev) != hipSuccess || hipSetDevice((int)dev) != hipSuccess) {
        delete o;
        return refuse(MLD_ERR_HIP, fn, ": the device of the context's stream is not usable");
    }
    o->device = (int)dev;
    const int rc = init(o);
    if (rc != MLD_OK) {
        const std::string text = std::string(": ") + o->err;
        o->stream = nullptr;  // (nothing of the object is in flight that the frees would not wait for)
        release_object(o);
        return refuse(rc, fn, text.c_str());
    }
    return o;
}

}  // namespace mld_batch
