// mld_labels.hip — per-track semantic labels by majority vote in a window of a label image, for a batch of sequences
// (include/mld.h, "mld_labels").
//
// matches_conversion_ros_tool's semantic_labels node (src/semantic_labels/semantic_labels.cpp:38-72): assignLabels takes
// the newest feature point of every track, counts the uchar labels of the mono8 image in
//   columns [max(0, p.x - w/2), min(cols, p.x + w/2))  x  rows [max(0, p.y - h/2), min(rows, p.y + h/2))
// (integer w/2, h/2: the window is 2*(w/2) x 2*(h/2), offset toward the upper left) and writes the most frequent one
// into TrackletWithOutlierFlag.label.  Here every sequence's tracks are answered by one launch.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream); it shares no internals
// with mld_api.hip or mld_tracks.hip.  Descriptor ring and object skeleton: ../batch/mld_batch_object.h.
//
// Two kernel shapes, chosen per call from the nominal window W x H = 2*(w/2) x 2*(h/2):
//   k_labels_row   W * H <= 16 (the default roi 5 x 5 counts 4 x 4 pixels).  A block answers 256 tracks, a wavefront 64:
//                  lane l computes the clipped window of track l, then in 16 rounds the four 16-lane rows of the
//                  wavefront take one track each, one pixel per lane (the 16 byte loads of a lane are all in flight
//                  before the first is used).  A lane's count is the number of lanes of its row with an equal label
//                  (15 row rotations), the winner the row maximum of (count << 8) | (255 - label).  No LDS; labels and
//                  votes are stored by the lane that owns the track, coalesced.
//   k_labels_wave  larger windows.  A block answers 32 tracks, a wavefront 8, one after the other: the 64 lanes stride
//                  over the clipped window, vote into the wavefront's own 256-bin LDS histogram and reduce the bins with
//                  the same key (64 bits wide: a window may hold 2^31 - 1 pixels).  The bins are cleared while they are
//                  reduced.
// In both, the key's low byte makes the smallest label win among equal counts, and a key of 0 is an empty window.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>

#include "../batch/mld_batch_object.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRowTracks = kBlock;   // tracks per block of k_labels_row: one per thread
constexpr int kWaveTracks = 32;      // tracks per block of k_labels_wave: 8 per wavefront
constexpr int kNoLabel = -2;         // matches_msg_conversions_ros/convert.hpp:53,97: a track nobody labelled

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct LbSeq {
    const uint8_t* img;
    const float* u;
    const float* v;
    int16_t* label;
    int32_t* votes;  // may be null
    int32_t n;       // tracks
    int32_t blk0;    // first block of the sequence in the launch
};
static_assert(sizeof(LbSeq) == 48, "48 bytes per sequence (DESIGN.md)");

struct LbGeom {
    int32_t rows, cols, stride;
    int32_t hw, hh;  // roi_width / 2, roi_height / 2
};

// The sequence a block belongs to: the last one whose first block is <= b (sequences without blocks share their
// successor's first block and are skipped).
__device__ __forceinline__ int seq_of_block(const LbSeq* __restrict__ desc, int n_seq, int b) {
    int lo = 0, hi = n_seq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// (int)x as C++ defines it; false where the conversion is undefined (NaN, inf, beyond int).  -2^31 is a float, the
// largest float below 2^31 is 2^31 - 128.
__device__ __forceinline__ bool trunc_to_int(float x, int& out) {
    const bool ok = x >= -2147483648.0f && x < 2147483648.0f;
    out = ok ? (int)x : 0;
    return ok;
}

// [max(0, p - half), min(size, p + half)) in exact arithmetic; an empty range comes back as (0, 0).
__device__ __forceinline__ void clip_range(int p, int half, int size, int& lo, int& len) {
    const long long a = std::max<long long>(0, (long long)p - half);
    const long long b = std::min<long long>(size, (long long)p + half);
    lo = b > a ? (int)a : 0;
    len = b > a ? (int)(b - a) : 0;
}

struct Window {
    int x0, y0, w, h;  // w == 0 && h == 0: empty
};

__device__ __forceinline__ Window window_of(float u, float v, const LbGeom& g) {
    Window win{0, 0, 0, 0};
    int px, py;
    const bool u_ok = trunc_to_int(u, px), v_ok = trunc_to_int(v, py);
    if (u_ok && v_ok) {
        clip_range(px, g.hw, g.cols, win.x0, win.w);
        clip_range(py, g.hh, g.rows, win.y0, win.h);
        if (win.w == 0 || win.h == 0) win = Window{0, 0, 0, 0};
    }
    return win;
}

// The value of the lane K places further on in this lane's row of 16 (wrapping inside the row).  Every lane of the
// wavefront must be active.
template <int K>
__device__ __forceinline__ int row_ror(int x) {
    static_assert(K >= 1 && K <= 15, "a rotation inside a row of 16");
    return __builtin_amdgcn_update_dpp(0, x, 0x120 + K, 0xf, 0xf, false);
}

template <int... K>
__device__ __forceinline__ int equal_in_row(int x, std::integer_sequence<int, K...>) {
    int c = 1;  // (the lane itself)
    ((c += row_ror<K + 1>(x) == x ? 1 : 0), ...);
    return c;
}

__device__ __forceinline__ int row_max(int x) {  // in every lane of the row
    x = std::max(x, row_ror<8>(x));
    x = std::max(x, row_ror<4>(x));
    x = std::max(x, row_ror<2>(x));
    return std::max(x, row_ror<1>(x));
}

__device__ __forceinline__ void store_result(const LbSeq& q, int i, int count, int label, int pixels) {
    q.label[i] = (int16_t)(count > 0 ? label : kNoLabel);
    if (q.votes) {
        q.votes[2 * (size_t)i + 0] = count;
        q.votes[2 * (size_t)i + 1] = pixels;
    }
}

// Nominal windows of at most 16 pixels: wn = 2 * hw columns, wn * 2 * hh <= 16.
__global__ __launch_bounds__(kBlock) void k_labels_row(const LbSeq* __restrict__ desc, int n_seq, LbGeom g) {
    const int s = seq_of_block(desc, n_seq, (int)blockIdx.x);
    const LbSeq q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kRowTracks + (int)threadIdx.x;
    const int lane = (int)threadIdx.x & 63;
    // this lane's own track (beyond the sequence: an empty window, nothing stored)
    Window mine{0, 0, 0, 0};
    if (i < q.n) mine = window_of(q.u[i], q.v[i], g);
    const int wn = 2 * g.hw;
    const int j = lane & 15;                                   // the pixel of the window this lane looks at
    const int dx = wn > 0 ? j % wn : 0, dy = wn > 0 ? j / wn : 0;
    const uint8_t* __restrict__ img = q.img;
    // round k: row r of the wavefront answers the track of lane 4 * k + r.  All 16 loads are issued before the first
    // is waited for.
    int lab[16];  // 256 = equal to no label: lanes outside the clipped window contribute nothing
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int src = 4 * k + (lane >> 4);
        const int x0 = __shfl(mine.x0, src), y0 = __shfl(mine.y0, src);
        const int wh = __shfl(mine.w | (mine.h << 8), src);  // (both <= 8 here)
        lab[k] = 256;
        if (dx < (wh & 255) && dy < (wh >> 8)) lab[k] = img[(size_t)(y0 + dy) * (size_t)g.stride + (size_t)(x0 + dx)];
    }
    int my_key = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int cnt = equal_in_row(lab[k], std::make_integer_sequence<int, 15>{});
        const int key = row_max(lab[k] < 256 ? (cnt << 8) | (255 - lab[k]) : 0);
        const int back = __shfl(key, (lane & 3) << 4);  // row r's answer to lane 4 * k + r
        if ((lane >> 2) == k) my_key = back;
    }
    if (i < q.n) store_result(q, i, my_key >> 8, 255 - (my_key & 255), mine.w * mine.h);
}

// Any window.
__global__ __launch_bounds__(kBlock) void k_labels_wave(const LbSeq* __restrict__ desc, int n_seq, LbGeom g) {
    __shared__ uint32_t bins_all[kBlock / 64][256];
    const int s = seq_of_block(desc, n_seq, (int)blockIdx.x);
    const LbSeq q = desc[s];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint32_t* bins = bins_all[wave];
    for (int b = lane; b < 256; b += 64) bins[b] = 0;
    const uint8_t* __restrict__ img = q.img;
    constexpr int kPerWave = kWaveTracks / (kBlock / 64);
    const int first = ((int)blockIdx.x - q.blk0) * kWaveTracks + wave * kPerWave;
    for (int t = 0; t < kPerWave; t++) {
        const int i = first + t;
        if (i >= q.n) break;  // (uniform in the wavefront)
        const Window win = window_of(q.u[i], q.v[i], g);  // (the same in every lane)
        const int total = win.w * win.h;                  // (< 2^31: the window lies inside the image)
        if (total == 0) {
            if (lane == 0) store_result(q, i, 0, 0, 0);
            continue;
        }
        // lane l takes the pixels l, l + 64, ... of the window in row-major order; (dx, dy) is carried along
        int dx = lane % win.w, dy = lane / win.w;
        const int step_x = 64 % win.w, step_y = 64 / win.w;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int base = 0; base < total; base += 64) {
            const bool inside = base + lane < total;  // (lane 0 always is)
            int lab = -1;
            if (inside) lab = img[(size_t)(win.y0 + dy) * (size_t)g.stride + (size_t)(win.x0 + dx)];
            const int lab0 = __builtin_amdgcn_readfirstlane(lab);
            const unsigned long long in = __ballot(inside);
            if (__ballot(inside && lab == lab0) == in) {  // one label in all 64 pixels (the usual case): one add
                if (lane == 0) atomicAdd(&bins[lab0], (uint32_t)__popcll(in));
            } else if (inside) {
                atomicAdd(&bins[lab], 1u);
            }
            dx += step_x;
            dy += step_y;
            if (dx >= win.w) {
                dx -= win.w;
                dy++;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned long long key = 0;
        for (int b = lane; b < 256; b += 64) {
            const uint32_t c = bins[b];
            bins[b] = 0;
            if (c) key = std::max(key, ((unsigned long long)c << 8) | (unsigned)(255 - b));
        }
        for (int off = 32; off > 0; off >>= 1) key = std::max(key, (unsigned long long)__shfl_xor((long long)key, off));
        if (lane == 0) store_result(q, i, (int)(key >> 8), 255 - (int)(key & 255), total);
    }
}

char g_error[512] = "";  // refusals without an object: mld_labels_last_error(NULL)

}  // namespace

struct mld_labels : mld_batch::Object {
    int n_seq = 0;
    mld_batch::DescRing<LbSeq> ring;
};

extern "C" {

mld_labels* mld_labels_create(mld_ctx* ctx, int n_seq, int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the size first: it is refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_labels_create: n_seq must be in 1 .. 65536";
        if (!ctx) return "mld_labels_create: null context";
        return nullptr;
    };
    auto init = [&](mld_labels* lb) {
        lb->n_seq = n_seq;
        return lb->ring.allocate(lb, n_seq);
    };
    return mld_batch::create_object<mld_labels>(g_error, "mld_labels_create", refusal(), ctx, status_out, init);
}

void mld_labels_destroy(mld_labels* lb) { mld_batch::destroy_object(lb); }

const char* mld_labels_last_error(const mld_labels* lb) { return lb ? lb->err.c_str() : g_error; }

int mld_labels_assign_device(mld_labels* lb, const uint8_t* const* label_image_dev, int rows, int cols, int row_stride_bytes,
                             int roi_width, int roi_height, const float* const* u, const float* const* v,
                             const int64_t* n_tracks, int16_t* const* label_out, int32_t* const* votes_out) {
    if (!lb) return mld_batch::no_object(g_error, "mld_labels_assign_device", "lb");
    if (rows < 1 || cols < 1) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: rows and cols must be >= 1");
    if ((int64_t)rows * cols > 0x7fffffff)
        return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: rows * cols must be below 2^31");
    if (row_stride_bytes < cols) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: row_stride_bytes must be >= cols");
    if (roi_width < 0 || roi_height < 0)
        return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: roi_width and roi_height must be >= 0");
    if (!label_image_dev) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: null table label_image_dev");
    if (!u || !v) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: null table u / v");
    if (!n_tracks) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: null table n_tracks");
    if (!label_out) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: null table label_out");
    const int S = lb->n_seq;
    for (int s = 0; s < S; s++) {
        if (n_tracks[s] < 0) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: negative n_tracks");
        if (n_tracks[s] > 0x7fffffff) return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: n_tracks must be below 2^31");
        if (n_tracks[s] > 0 && (!label_image_dev[s] || !u[s] || !v[s] || !label_out[s]))
            return fail(lb, MLD_ERR_INVALID_ARG, "mld_labels_assign_device: null array (label_image_dev, u, v or label_out) of a sequence with tracks");
    }
    // the shape: one row of 16 lanes per track while the nominal window has at most 16 pixels
    const int hw = roi_width / 2, hh = roi_height / 2;
    const bool row_shape = (int64_t)(2 * (int64_t)hw) * (2 * (int64_t)hh) <= 16;
    const int per_block = row_shape ? kRowTracks : kWaveTracks;
    int64_t blocks = 0;
    for (int s = 0; s < S; s++) {
        LbSeq& q = lb->ring.stage[(size_t)s];
        q.img = label_image_dev[s];
        q.u = u[s];
        q.v = v[s];
        q.label = label_out[s];
        q.votes = votes_out ? votes_out[s] : nullptr;
        q.n = (int32_t)n_tracks[s];
        q.blk0 = (int32_t)blocks;
        blocks += (n_tracks[s] + per_block - 1) / per_block;
        if (blocks > 0x7fffffff) return fail(lb, MLD_ERR_CAPACITY, "mld_labels_assign_device: more than 2^31 blocks in one launch");
    }
    if (blocks == 0) return MLD_OK;
    MLD_HIP(lb, hipSetDevice(lb->device));
    const int rc = lb->ring.upload(lb);
    if (rc) return rc;
    const LbGeom g{rows, cols, row_stride_bytes, hw, hh};
    if (row_shape)
        hipLaunchKernelGGL(k_labels_row, dim3((unsigned)blocks), dim3(kBlock), 0, lb->stream, lb->ring.d_desc.get(), S, g);
    else
        hipLaunchKernelGGL(k_labels_wave, dim3((unsigned)blocks), dim3(kBlock), 0, lb->stream, lb->ring.d_desc.get(), S, g);
    MLD_HIP(lb, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
