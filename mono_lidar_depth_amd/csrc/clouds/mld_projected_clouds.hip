// mld_projected_clouds.hip — the frame's PointcloudData (monolidar_fusion PointcloudData.h:13-68, filled by
// DepthEstimator::Transform_Cloud_LidarToImage, DepthEstimator.cpp:155-218, and NeighborFinderPixel.cpp:38-55) for a batch
// of sequences in one call (include/mld.h, "mld_projected_clouds"): the visible list (getPointsCloudImageCs), _pointIndex,
// getPointDepthCamVisible, the camera-frame cloud (getCloudCameraCs) and the reference-format pixel map.  No frame slot is
// involved, clouds are read where they lie, nothing is allocated per call and nothing comes back to the host.
//
// Up to four launches, ordered by kernel boundaries alone (no flags, no waiting between blocks):
//   k_pc_fill   (only if a map is asked for) grid (sequence, cells): -1 into every cell of the maps
//   k_pc_pass   grid (sequence, 1024 points): exact transform and projection; the visibility ballot as one 64-bit word per
//               64 points and one count per 1024 points, both in the object's device scratch; cam_out where asked for
//   k_pc_scan   one block per sequence: exclusive prefix of the counts, in place; the total is n_visible
//   k_pc_write  grid as the pass: rank of a visible point = block base + popcounts of the block's earlier words + prefix
//               within its word.  Only the visible lanes load their record again and project it again - the arithmetic is
//               deterministic f64, so they get what the pass got - and store uv, index and depth where rank < capacity; a
//               point with z_cam > 0 puts its rank into its map cell by atomicMin on the cell as uint32 (the -1 of the fill
//               is 0xFFFFFFFF): the smallest visible index wins, which is the reference's "first wins".
// Nothing of the size of the cloud is stored between the passes (the ballots are one bit per point).
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring, object skeleton and compaction scratch: ../batch/mld_batch_object.h; the compaction's device
// pieces, load_xyz and to_camera: ../batch/mld_batch_device.h).  The results are nevertheless bit for bit those of the
// one-slot getters (tests/test_projected_clouds_gpu.py pins that): the shared to_camera and to_image below restate,
// operation for operation, that path's transform and projection, in f64 from the float coordinates, and this unit
// is compiled without contraction like the rest of the library.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;
constexpr int kGroupsPerWave = 4;                  // consecutive groups of 64 points a wavefront takes
constexpr int kChunk = kBlock * kGroupsPerWave;    // 1024 points = 16 groups per block
constexpr int kGroupsPerChunk = kChunk / kWave;
constexpr int kFillPerThread = 4;                  // cells a thread of k_pc_fill clears per step
constexpr unsigned kFillMaxBlocks = 4096;          // per sequence; the blocks stride over larger maps

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct PcSeq {
    const unsigned char* cloud;
    double* uv;       // 2 x capacity, null: capacity 0
    int32_t* index;   // capacity
    double* depth;    // capacity, or null
    double* cam;      // 3 x n, or null
    int32_t* map;     // W * H, or null
    int32_t n;
    int32_t capacity;  // min(capacity[s], n[s]): a rank is below n
};
static_assert(sizeof(PcSeq) == 56, "56 bytes per sequence (DESIGN.md)");

struct PcCalib {
    double T[12];  // lidar -> camera, row-major 3x4
    double f, cu, cv;
    int32_t W, H;
};

// camera_pinhole.h:88-90: q = K p with all nine products, hnormalized.
__device__ __forceinline__ void to_image(const PcCalib& c, V3 p, double& u, double& v) {
    const double q0 = (c.f * p.x + 0.0 * p.y) + c.cu * p.z;
    const double q1 = (0.0 * p.x + c.f * p.y) + c.cv * p.z;
    const double q2 = (0.0 * p.x + 0.0 * p.y) + 1.0 * p.z;
    u = q0 / q2;
    v = q1 / q2;
}

// DepthEstimator.cpp:184-207: in range (inclusive bounds, camera_pinhole.h:93-95) and within the strict bounds.  NaN and
// inf fail the comparisons; so does z_cam == 0 (u, v = inf or NaN).  A point behind the camera may pass.
__device__ __forceinline__ bool is_visible(const PcCalib& c, double u, double v) {
    const double Wd = (double)c.W, Hd = (double)c.H;
    const bool inr = (u >= 0.) && (u <= Wd) && (v >= 0.) && (v <= Hd);
    const bool strict = (u > 0.) && (u < Wd) && (v > 0.) && (v < Hd);
    return inr && strict;
}

// NeighborFinderPixel.cpp:38 setConstant(POINT_NOT_DEFINED): every cell of every map that was asked for.  Grid (sequence,
// blocks striding over the cells); a map needs 4-byte alignment only, so the 16-byte stores are declared that way.
typedef int int4v __attribute__((ext_vector_type(4)));
typedef int4v int4u __attribute__((aligned(4)));

__global__ __launch_bounds__(kBlock) void k_pc_fill(const PcSeq* __restrict__ desc, long long cells) {
    int32_t* const map = desc[blockIdx.x].map;
    if (!map) return;  // (uniform in the block)
    MLD_BATCH_GLOBAL int32_t* m = as_global(map);
    const long long step = (long long)gridDim.y * kBlock * kFillPerThread;
    for (long long i = ((long long)blockIdx.y * kBlock + threadIdx.x) * kFillPerThread; i < cells; i += step) {
        if (i + kFillPerThread <= cells) {
            *(MLD_BATCH_GLOBAL int4u*)(m + i) = int4v{-1, -1, -1, -1};
        } else {
            for (long long j = i; j < cells; j++) m[j] = -1;
        }
    }
}

// Grid (sequence, chunk of 1024 points).  gm: one 64-bit visibility mask per 64 points, cpre[c + 1]: the visible points of
// chunk c (k_pc_scan makes them a prefix).
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_pc_pass(const PcSeq* __restrict__ desc, PcCalib c,
                                                   unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                   int* __restrict__ cpre_all, long long chunks_per_seq) {
    __shared__ int wsum[kBlock / kWave];
    const PcSeq q = desc[blockIdx.x];
    const int n = q.n;
    if ((int)blockIdx.y * kChunk >= n) return;  // (uniform in the block; max_points < 2^23: no overflow)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int first = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave * kWave;  // the wavefront's first point
    unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    float x[kGroupsPerWave], y[kGroupsPerWave], z[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        x[k] = y[k] = z[k] = 0.f;
        if (i < n) load_xyz<kStride>(q.cloud, i, x[k], y[k], z[k]);
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave, i = i0 + lane;
        const V3 pc = to_camera(c.T, (double)x[k], (double)y[k], (double)z[k]);
        double u, v;
        to_image(c, pc, u, v);
        const bool f = (i < n) && is_visible(c, u, v);
        if (cam && i < n) {
            cam[3 * (size_t)i] = pc.x;
            cam[3 * (size_t)i + 1] = pc.y;
            cam[3 * (size_t)i + 2] = pc.z;
        }
        const unsigned long long m = __ballot(f);
        if (lane == 0 && i0 < n) *as_global(gm + (i0 >> 6)) = m;
        cnt += (int)__popcll(m);
    }
    if (lane == 0) wsum[wave] = cnt;
    chunk_count(wsum, cpre_all, chunks_per_seq);
}

// Exclusive prefix over the chunk counts of a sequence, in place: cpre[c] = visible points ahead of chunk c; the total
// goes to n_visible[s].  The loop carries the sum over any number of chunks (up to 8192).
__global__ __launch_bounds__(256) void k_pc_scan(const PcSeq* __restrict__ desc, int* __restrict__ cpre_all,
                                                long long chunks_per_seq, long long* __restrict__ n_visible) {
    const int n = desc[blockIdx.x].n;
    const int NC = (n + kChunk - 1) / kChunk;
    const int total = scan_chunk_counts(cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1), NC);
    if (threadIdx.x == 0) n_visible[blockIdx.x] = (long long)total;
}

// Grid as the pass.  Every wavefront reads the (up to 16) masks of its block, one per lane, and scans their counts; the
// visible lanes of its four groups then do the work.
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_pc_write(const PcSeq* __restrict__ desc, PcCalib c,
                                                    const unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                    const int* __restrict__ cpre_all, long long chunks_per_seq) {
    const PcSeq q = desc[blockIdx.x];
    const int n = q.n;
    const int b = (int)blockIdx.y;
    if (b * kChunk >= n) return;  // (uniform in the block)
    const int* __restrict__ cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1);
    const int base = cpre[b];
    if (cpre[b + 1] == base) return;  // no visible point in this chunk (uniform in the block)
    const unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int G = (n + kWave - 1) / kWave;
    const int g_mine = b * kGroupsPerChunk + lane;  // lanes 0..15: the masks of the block
    const unsigned long long mine = (lane < kGroupsPerChunk && g_mine < G) ? gm[g_mine] : 0ull;
    MLD_BATCH_GLOBAL double* uv = as_global(q.uv);
    MLD_BATCH_GLOBAL int32_t* index = as_global(q.index);
    MLD_BATCH_GLOBAL double* depth = as_global(q.depth);
    // (the cross-lane reads while every lane is here)
    unsigned lo[kGroupsPerWave], hi[kGroupsPerWave];
    int first_rank[kGroupsPerWave];
    group_ranks<kGroupsPerChunk>(mine, base, lane, wave, lo, hi, first_rank);
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const unsigned long long m = ((unsigned long long)hi[k] << 32) | lo[k];
        if (!((m >> lane) & 1ull)) continue;  // (a set bit is a point below n)
        const int rank = first_rank[k] + lane_rank(lo[k], hi[k]);
        const int i = ((b * kGroupsPerChunk + wave * kGroupsPerWave + k) << 6) + lane;
        float x, y, z;
        load_xyz<kStride>(q.cloud, i, x, y, z);
        const V3 pc = to_camera(c.T, (double)x, (double)y, (double)z);
        double u, v;
        to_image(c, pc, u, v);
        if (rank < q.capacity) {
            uv[2 * (size_t)rank] = u;
            uv[2 * (size_t)rank + 1] = v;
            index[rank] = i;
            if (depth) depth[rank] = pc.z;
        }
        // NeighborFinderPixel.cpp:41,51-54: truncation, z > 0, first wins.  0 < u < W and 0 < v < H: the cell is in range.
        if (q.map && pc.z > 0.)
            __hip_atomic_fetch_min(as_global(reinterpret_cast<unsigned int*>(q.map)) + ((size_t)(int)u + (size_t)(int)v * (size_t)c.W),
                                   (unsigned)rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

char g_error[512] = "";  // refusals without an object: mld_projected_clouds_last_error(NULL)

}  // namespace

struct mld_projected_clouds : mld_batch::Object {
    int n_seq = 0;
    int64_t max_points = 0;
    PcCalib calib{};
    CompactScratch scratch;  // visibility mask per group; visible points ahead of every chunk (+ the total)
    mld_batch::DescRing<PcSeq> ring;
};

namespace {

int allocate(mld_projected_clouds* pc) {
    const int rc = pc->ring.allocate(pc, pc->n_seq);
    if (rc) return rc;
    return pc->scratch.allocate(pc, pc->n_seq, pc->max_points, kChunk, 1);
}

template <int kStride>
void launch_all(mld_projected_clouds* pc, int chunks, bool any_map, int64_t* n_visible) {
    const unsigned S = (unsigned)pc->n_seq;
    const CompactScratch& cs = pc->scratch;
    if (any_map) {
        const long long cells = (long long)pc->calib.W * pc->calib.H;
        const long long per_block = (long long)kBlock * kFillPerThread;
        const long long blocks = (cells + per_block - 1) / per_block;
        hipLaunchKernelGGL(k_pc_fill, dim3(S, blocks < (long long)kFillMaxBlocks ? (unsigned)blocks : kFillMaxBlocks), dim3(kBlock),
                           0, pc->stream, pc->ring.d_desc.get(), cells);
    }
    if (chunks > 0)
        hipLaunchKernelGGL(k_pc_pass<kStride>, dim3(S, (unsigned)chunks), dim3(kBlock), 0, pc->stream, pc->ring.d_desc.get(), pc->calib,
                           cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
    hipLaunchKernelGGL(k_pc_scan, dim3(S), dim3(256), 0, pc->stream, pc->ring.d_desc.get(), cs.d_cpre.get(), cs.chunks_per_seq,
                       reinterpret_cast<long long*>(n_visible));
    if (chunks > 0)
        hipLaunchKernelGGL(k_pc_write<kStride>, dim3(S, (unsigned)chunks), dim3(kBlock), 0, pc->stream, pc->ring.d_desc.get(), pc->calib,
                           cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
}

}  // namespace

extern "C" {

mld_projected_clouds* mld_projected_clouds_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_camera* camera,
                                                  const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_projected_clouds_create: n_seq must be in 1 .. 65536";
        if (max_points < 1 || max_points > kMaxPoints) return "mld_projected_clouds_create: max_points must be in 1 .. 8388607";
        if (!ctx) return "mld_projected_clouds_create: null context";
        if (!camera) return "mld_projected_clouds_create: null camera";
        if (!T_cam_lidar) return "mld_projected_clouds_create: null T_cam_lidar";
        if (camera->width < 1 || camera->height < 1) return "mld_projected_clouds_create: camera width and height must be >= 1";
        if ((int64_t)camera->width * camera->height > 2147483647)
            return "mld_projected_clouds_create: camera width * height must be below 2^31";
        return nullptr;
    };
    auto init = [&](mld_projected_clouds* pc) {
        pc->n_seq = n_seq;
        pc->max_points = max_points;
        for (int t = 0; t < 12; t++) pc->calib.T[t] = T_cam_lidar[t];
        pc->calib.f = camera->focal_length;
        pc->calib.cu = camera->principal_point_x;
        pc->calib.cv = camera->principal_point_y;
        pc->calib.W = camera->width;
        pc->calib.H = camera->height;
        return allocate(pc);
    };
    return mld_batch::create_object<mld_projected_clouds>(g_error, "mld_projected_clouds_create", refusal(), ctx, status_out, init);
}

void mld_projected_clouds_destroy(mld_projected_clouds* pc) { mld_batch::destroy_object(pc); }

const char* mld_projected_clouds_last_error(const mld_projected_clouds* pc) { return pc ? pc->err.c_str() : g_error; }

int mld_projected_clouds_export_device(mld_projected_clouds* pc, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                                       const int64_t* capacity, int64_t* n_visible_out_dev, double* const* uv_out,
                                       int32_t* const* index_out, double* const* depth_out, double* const* cam_out,
                                       int32_t* const* map_out) {
    if (!pc) return no_object(g_error, "mld_projected_clouds_export_device", "pc");
#define PC_REFUSE(text) return fail(pc, MLD_ERR_INVALID_ARG, "mld_projected_clouds_export_device: " text)
    if (!pts_dev) PC_REFUSE("null table pts_dev");
    if (!n) PC_REFUSE("null table n");
    if (!capacity) PC_REFUSE("null table capacity");
    if (!n_visible_out_dev) PC_REFUSE("null array n_visible_out_dev");
    if (!uv_out) PC_REFUSE("null table uv_out");
    if (!index_out) PC_REFUSE("null table index_out");
    if (stride_bytes != 16 && stride_bytes != 32) PC_REFUSE("stride_bytes must be 16 or 32");
    const int S = pc->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if (n[s] < 0) PC_REFUSE("negative n");
        if (capacity[s] < 0) PC_REFUSE("negative capacity");
        if (n[s] > pc->max_points)
            return fail(pc, MLD_ERR_CAPACITY, "mld_projected_clouds_export_device: n exceeds the max_points of the object");
        if (n[s] > 0) {
            if (!pts_dev[s]) PC_REFUSE("null array pts_dev of a sequence with points");
            if (misaligned(pts_dev[s], 3u)) PC_REFUSE("pts_dev must be 4-byte aligned");
            if (capacity[s] > 0) {
                if (!uv_out[s]) PC_REFUSE("null array uv_out of a sequence with points and capacity");
                if (!index_out[s]) PC_REFUSE("null array index_out of a sequence with points and capacity");
            }
        }
        if (n[s] > longest) longest = n[s];
    }
#undef PC_REFUSE
    bool any_map = false;
    for (int s = 0; s < S; s++) {
        PcSeq& q = pc->ring.stage[(size_t)s];
        const int64_t cap = capacity[s] < n[s] ? capacity[s] : n[s];
        q.cloud = static_cast<const unsigned char*>(pts_dev[s]);
        q.uv = cap > 0 ? uv_out[s] : nullptr;
        q.index = cap > 0 ? index_out[s] : nullptr;
        q.depth = (cap > 0 && depth_out) ? depth_out[s] : nullptr;
        q.cam = (n[s] > 0 && cam_out) ? cam_out[s] : nullptr;
        q.map = map_out ? map_out[s] : nullptr;
        q.n = (int32_t)n[s];
        q.capacity = (int32_t)cap;
        any_map = any_map || q.map;
    }
    MLD_HIP(pc, hipSetDevice(pc->device));
    const int rc = pc->ring.upload(pc);
    if (rc) return rc;
    const int chunks = (int)((longest + kChunk - 1) / kChunk);  // (<= 8192)
    with_stride(stride_bytes, [&](auto stride) { launch_all<decltype(stride)::value>(pc, chunks, any_map, n_visible_out_dev); });
    MLD_HIP(pc, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
