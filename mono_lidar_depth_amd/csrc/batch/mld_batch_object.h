// mld_batch_object.h — the host side the batch objects on top of the public C-ABI have in common (mld_tracks, mld_labels,
// mld_semantic_planes, mld_ransac_planes, mld_projected_clouds, mld_depth_reports, mld_plane_inliers, mld_feature_traces;
// each a translation unit of its own that includes this header, include/mld.h and - for what their kernels share -
// mld_batch_device.h only):
//   Object         the fields every object has (context, stream, device, last error), fail() and the MLD_HIP check on them
//   DescRing<D>    the per-call table of n_seq descriptors: staged on the host, copied into one of kGens pinned
//                  generations and moved to device memory by a kernel on the object's stream
//   CompactScratch the device scratch of a pass / scan / write stream compaction (mld_batch_device.h) and its sizes
//   create_object / release_object / destroy_object   the skeleton of mld_*_create and mld_*_destroy
//   no_object, misaligned, with_stride   the refusal of a call on no object, the alignment test, the 16 / 32 dispatch
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

template <typename Desc>
struct DescRing {
    static_assert(sizeof(Desc) % 4 == 0, "the upload kernel moves 32-bit words");
    Desc* d_desc = nullptr;            // what the kernels of a call read
    unsigned char* up_base = nullptr;  // pinned: kGens generations of n_seq descriptors
    size_t gen_bytes = 0;
    hipEvent_t up_ev[kGens] = {};      // recorded behind the upload kernel that reads the generation
    bool up_busy[kGens] = {};
    int up_next = 0;
    std::vector<Desc> stage;           // the next call's descriptors, filled by the caller

    int allocate(Object* o, int n_seq) {
        stage.assign((size_t)n_seq, Desc{});
        gen_bytes = (size_t)n_seq * sizeof(Desc);
        MLD_HIP(o, hipMalloc((void**)&d_desc, gen_bytes));
        MLD_HIP(o, hipHostMalloc((void**)&up_base, gen_bytes * kGens, hipHostMallocDefault));
        for (int g = 0; g < kGens; g++) MLD_HIP(o, hipEventCreateWithFlags(&up_ev[g], hipEventDisableTiming));
        return MLD_OK;
    }

    // The staged descriptors to the device on the object's stream; `stage` may be rewritten as soon as this returns.
    int upload(Object* o) {
        const int g = up_next;
        if (up_busy[g]) MLD_HIP(o, hipEventSynchronize(up_ev[g]));  // (only when kGens uploads are still queued)
        unsigned char* pinned = up_base + (size_t)g * gen_bytes;
        std::memcpy(pinned, stage.data(), gen_bytes);
        const int words = (int)(gen_bytes / 4);
        hipLaunchKernelGGL(k_batch_upload, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, o->stream,
                           reinterpret_cast<uint32_t*>(d_desc), reinterpret_cast<const uint32_t*>(pinned), words);
        MLD_HIP(o, hipGetLastError());
        MLD_HIP(o, hipEventRecord(up_ev[g], o->stream));
        up_busy[g] = true;
        up_next = (g + 1) % kGens;
        return MLD_OK;
    }

    // After the stream has been synchronised (release_object).
    void release() {
        if (d_desc) (void)hipFree(d_desc);
        if (up_base) (void)hipHostFree(up_base);
        for (int g = 0; g < kGens; g++)
            if (up_ev[g]) (void)hipEventDestroy(up_ev[g]);
    }
};

// The device scratch of a stream compaction over sequences of up to max_items items: one 64-bit mask per group of 64
// items, and per chunk of `chunk` items (+ 1: the total) `columns` counts side by side.
struct CompactScratch {
    unsigned long long* d_gm = nullptr;
    int* d_cpre = nullptr;
    long long groups_per_seq = 0;
    long long chunks_per_seq = 0;

    int allocate(Object* o, int n_seq, int64_t max_items, int chunk, int columns, bool masks = true) {
        groups_per_seq = (long long)((max_items + 63) / 64);
        chunks_per_seq = (long long)((max_items + chunk - 1) / chunk);
        if (masks) MLD_HIP(o, hipMalloc((void**)&d_gm, (size_t)n_seq * (size_t)groups_per_seq * sizeof(unsigned long long)));
        MLD_HIP(o, hipMalloc((void**)&d_cpre, (size_t)n_seq * (size_t)(chunks_per_seq + 1) * (size_t)columns * sizeof(int)));
        return MLD_OK;
    }

    // After the stream has been synchronised (release_object).
    void release() {
        if (d_gm) (void)hipFree(d_gm);
        if (d_cpre) (void)hipFree(d_cpre);
    }
};

// Obj: an Object with a member `ring`.  free_own(obj) frees the device memory the object allocated besides its ring.
template <typename Obj, typename FreeOwn>
void release_object(Obj* o, FreeOwn free_own) {
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    free_own(o);
    o->ring.release();
    delete o;
}

template <typename Obj, typename FreeOwn>
void destroy_object(Obj* o, FreeOwn free_own) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    release_object(o, free_own);
}

// mld_*_create behind the argument checks: `refusal` is the caller's verdict on its arguments (sizes first, then the
// context, then the rest; null: none), `no_object_error` its string for mld_*_last_error(NULL).  init(obj) fills in the
// object's own fields and allocates, the ring included, on the stream's device.
template <typename Obj, typename Init, typename FreeOwn>
Obj* create_object(char (&no_object_error)[512], const char* fn, const char* refusal, mld_ctx* ctx, int* status_out, Init init,
                   FreeOwn free_own) {
    auto refuse = [&](int code, const char* prefix, const char* text) -> Obj* {
        std::snprintf(no_object_error, sizeof(no_object_error), "%s%s", prefix, text);
        if (status_out) *status_out = code;
        return nullptr;
    };
    if (status_out) *status_out = MLD_OK;
    if (refusal) return refuse(MLD_ERR_INVALID_ARG, "", refusal);
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
        release_object(o, free_own);
        return refuse(rc, fn, text.c_str());
    }
    return o;
}

}  // namespace mld_batch
