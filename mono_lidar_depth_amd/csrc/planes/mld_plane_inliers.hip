// mld_plane_inliers.hip — what the reference keeps on a frame's ground plane besides its coefficients, for a batch of
// sequences in one call (include/mld.h, "mld_plane_inliers"): the ascending list of inlier indices
// (GroundPlane::getInlinersIndex, RansacPlane.h:109), the lidar-frame float matrix of the inliers
// (GroundPlane::getMatrixFromIndices, RansacPlane.cpp:142-151) and the camera-frame inlier cloud filtered by
// ransac_plane_use_camx_treshold / ransac_plane_treshold_camx (DepthEstimator::getCloudRansacPlane, DepthEstimator.cpp:
// 294-308,396-398).  The input is the inlier bitmask the two batch estimators write (mld_semantic_planes,
// mld_ransac_planes).  No frame slot is involved, clouds and masks are read where they lie, nothing is allocated per call
// and nothing comes back to the host.
//
// Up to three launches, ordered by kernel boundaries alone (no flags, no waiting between blocks):
//   k_pi_pass   grid (sequence, 1024 points): the block's 32 mask words with 32-bit loads, the bits at and beyond n
//               cleared; the inlier count per 1024 points.  With the camx filter on, the lanes whose bit is set - and only
//               they - load their record, transform x and ballot fabs(x_cam) <= threshold into a second 64-bit word per 64
//               points, and the block counts those as well; the second word of a group without an inlier is neither
//               written here nor read later.  With the filter off neither exists: cloud rank = inlier rank.
//   k_pi_scan   one block per sequence: exclusive prefixes of both counts, in place; the whole counts record
//   k_pi_write  grid as the pass: rank = block base + popcounts of the block's earlier words + prefix within the word, once
//               per rank kind.  Only inlier lanes with something to store load their record (index_out alone needs none)
//               and store index / lidar / cam below the capacity.
// The work is bound by the masks, not by the clouds: a block whose chunk holds no inlier reads 128 bytes of mask in the
// pass, two counts in the write, and nothing of the cloud.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring, object skeleton and compaction scratch: ../batch/mld_batch_object.h; the compaction's device
// pieces, load_xyz and to_camera: ../batch/mld_batch_device.h).  The results are nevertheless bit for bit those of the
// one-slot getters (tests/test_plane_inliers_gpu.py pins that): the shared to_camera restates, operation for operation,
// that path's transform, in f64 from the float coordinates, and this unit is compiled without contraction like the rest
// of the library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;
constexpr int kGroupsPerWave = 4;                  // consecutive groups of 64 points a wavefront takes
constexpr int kChunk = kBlock * kGroupsPerWave;    // 1024 points = 16 groups = 32 mask words per block
constexpr int kGroupsPerChunk = kChunk / kWave;
constexpr int kWordsPerWave = 2 * kGroupsPerWave;  // 32-bit mask words of a wavefront's groups
constexpr int kWordsPerChunk = 2 * kGroupsPerChunk;

static_assert(sizeof(mld_plane_inlier_counts) == 16, "two int64 (include/mld.h)");

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct PiSeq {
    const unsigned char* cloud;
    const uint32_t* mask;  // ceil(n / 32) words
    int32_t* index;        // capacity, null: capacity 0
    float* lidar;          // 3 x capacity, or null
    double* cam;           // 3 x capacity, or null
    int32_t n;
    int32_t capacity;  // min(capacity[s], n[s]): a rank is below n
};
static_assert(sizeof(PiSeq) == 48, "48 bytes per sequence (DESIGN.md)");

struct PiCalib {
    double T[12];  // lidar -> camera, row-major 3x4
    double thr;    // ransac_plane_treshold_camx
    int32_t use;   // ransac_plane_use_camx_treshold
};

// Mask word w of a sequence of n points (w < ceil(n / 32)), the bits at and beyond n cleared: a caller's own mask may
// carry anything there.
__device__ __forceinline__ unsigned load_word(const uint32_t* __restrict__ mask, int w, int n) {
    unsigned word = as_global(mask)[w];
    const int left = n - (w << 5);  // >= 1
    if (left < 32) word &= (1u << left) - 1u;
    return word;
}

// Grid (sequence, chunk of 1024 points).  cpre[2 (c + 1)], cpre[2 (c + 1) + 1]: the inliers of chunk c and those of them
// that pass the filter (k_pi_scan makes them prefixes); gm: the filter's ballot, one 64-bit word per 64 points.  Both
// second things only with the filter on.
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_pi_pass(const PiSeq* __restrict__ desc, PiCalib c,
                                                   unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                   int* __restrict__ cpre_all, long long chunks_per_seq) {
    __shared__ int wsum[2][kBlock / kWave];
    const PiSeq q = desc[blockIdx.x];
    const int n = q.n;
    if ((int)blockIdx.y * kChunk >= n) return;  // (uniform in the block; max_points < 2^23: no overflow)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int g0 = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave;  // the wavefront's first group
    const int W = (n + 31) >> 5;
    const int w = 2 * g0 + lane;  // lanes 0..7: the words of the wavefront
    const unsigned word = (lane < kWordsPerWave && w < W) ? load_word(q.mask, w, n) : 0u;
    // (the cross-lane reads while every lane is here)
    unsigned lo[kGroupsPerWave], hi[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        lo[k] = (unsigned)__shfl((int)word, 2 * k);
        hi[k] = (unsigned)__shfl((int)word, 2 * k + 1);
    }
    int cnt_in = 0, cnt_cl = 0;
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const unsigned long long m = ((unsigned long long)hi[k] << 32) | lo[k];
        cnt_in += (int)__popcll(m);
        if (!c.use || m == 0ull) continue;  // (uniform in the wavefront)
        bool f = false;
        if ((m >> lane) & 1ull) {  // (a set bit is a point below n)
            float x, y, z;
            load_xyz<kStride>(q.cloud, ((g0 + k) << 6) + lane, x, y, z);
            const V3 pc = to_camera(c.T, (double)x, (double)y, (double)z);
            f = fabs(pc.x) <= c.thr;  // NaN fails (DepthEstimator.cpp:300-307)
        }
        const unsigned long long mc = __ballot(f);
        if (lane == 0) *as_global(gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq + (size_t)(g0 + k)) = mc;
        cnt_cl += (int)__popcll(mc);
    }
    if (lane == 0) {
        wsum[0][wave] = cnt_in;
        wsum[1][wave] = cnt_cl;
    }
    __syncthreads();
    if (threadIdx.x < 2 && (threadIdx.x == 0 || c.use)) {
        int t = 0;
#pragma unroll
        for (int v = 0; v < kBlock / kWave; v++) t += wsum[threadIdx.x][v];
        *as_global(cpre_all + ((size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) + blockIdx.y + 1) * 2 + threadIdx.x) = t;
    }
}

// Exclusive prefixes over the chunk counts of a sequence, in place: cpre[2 c] = inliers ahead of chunk c, cpre[2 c + 1] =
// points of the cloud ahead of it (with the filter on); the totals are the counts record.  The loop carries the sums over
// any number of chunks (up to 8192).
__global__ __launch_bounds__(256) void k_pi_scan(const PiSeq* __restrict__ desc, int use, int* __restrict__ cpre_all,
                                                long long chunks_per_seq, long long* __restrict__ counts) {
    __shared__ int wsum[2][256 / kWave];
    const int n = desc[blockIdx.x].n;
    const int NC = (n + kChunk - 1) / kChunk;
    int* __restrict__ cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) * 2;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    if (tid < 2) cpre[tid] = 0;
    int carry_in = 0, carry_cl = 0;
    for (int c0 = 0; c0 < NC; c0 += 256) {  // (uniform)
        const int c = c0 + tid;
        const IntPair incl =
            scan_inclusive<kWave>(c < NC ? cpre[2 * (c + 1)] : 0, (use && c < NC) ? cpre[2 * (c + 1) + 1] : 0, lane);
        const int incl_in = incl.a, incl_cl = incl.b;
        if (lane == kWave - 1) {
            wsum[0][w] = incl_in;
            wsum[1][w] = incl_cl;
        }
        __syncthreads();
        int off_in = carry_in, off_cl = carry_cl, total_in = 0, total_cl = 0;
#pragma unroll
        for (int k = 0; k < 256 / kWave; k++) {
            off_in += k < w ? wsum[0][k] : 0;
            off_cl += k < w ? wsum[1][k] : 0;
            total_in += wsum[0][k];
            total_cl += wsum[1][k];
        }
        if (c < NC) {
            cpre[2 * (c + 1)] = off_in + incl_in;
            if (use) cpre[2 * (c + 1) + 1] = off_cl + incl_cl;
        }
        carry_in += total_in;
        carry_cl += total_cl;
        __syncthreads();
    }
    if (tid < 2)  // n_inliers, n_cloud
        *as_global(counts + (size_t)blockIdx.x * 2 + tid) = (long long)((tid == 1 && use) ? carry_cl : carry_in);
}

// Grid as the pass.  Every wavefront reads the (up to 32) mask words of its block, one per lane, and scans their counts;
// with the filter on likewise the (up to 16) words of the filter's ballot.  The inlier lanes of its four groups then do
// the work.
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_pi_write(const PiSeq* __restrict__ desc, PiCalib c,
                                                    const unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                    const int* __restrict__ cpre_all, long long chunks_per_seq) {
    const PiSeq q = desc[blockIdx.x];
    const int n = q.n;
    const int b = (int)blockIdx.y;
    if (b * kChunk >= n) return;  // (uniform in the block)
    const int* __restrict__ cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) * 2;
    const int base_in = cpre[2 * b];
    if (cpre[2 * (b + 1)] == base_in) return;  // no inlier in this chunk (uniform in the block)
    const int base_cl = c.use ? cpre[2 * b + 1] : base_in;  // (<= base_in)
    const bool want_cam = q.cam != nullptr && base_cl < q.capacity;
    if (base_in >= q.capacity && !want_cam) return;  // nothing of this chunk is stored (uniform in the block)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int W = (n + 31) >> 5;
    const int w_mine = b * kWordsPerChunk + lane;  // lanes 0..31: the words of the block
    const unsigned word = (lane < kWordsPerChunk && w_mine < W) ? load_word(q.mask, w_mine, n) : 0u;
    const int pop = (int)__popc(word);
    const int ahead_in = scan_inclusive<kWordsPerChunk>(pop, lane) - pop;  // inliers of the block ahead of this lane's word
    // lanes 0..15: the filter's ballot of the block's groups that have an inlier
    const int pair = (lane & (kGroupsPerChunk - 1)) * 2;
    const unsigned own = (unsigned)__shfl((int)word, pair) | (unsigned)__shfl((int)word, pair + 1);
    unsigned long long mine_cl = 0ull;
    if (c.use && lane < kGroupsPerChunk && own != 0u)
        mine_cl = *as_global(gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq + (size_t)(b * kGroupsPerChunk + lane));
    const int pop_cl = (int)__popcll(mine_cl);
    const int ahead_cl = scan_inclusive<kGroupsPerChunk>(pop_cl, lane) - pop_cl;  // points of the cloud ahead of this lane's group
    const unsigned cl_lo = (unsigned)mine_cl, cl_hi = (unsigned)(mine_cl >> 32);
    MLD_BATCH_GLOBAL int32_t* index = as_global(q.index);
    MLD_BATCH_GLOBAL float* lidar = as_global(q.lidar);
    MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    // (the cross-lane reads while every lane is here)
    unsigned lo[kGroupsPerWave], hi[kGroupsPerWave], flo[kGroupsPerWave], fhi[kGroupsPerWave];
    int first_in[kGroupsPerWave], first_cl[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int gl = wave * kGroupsPerWave + k;  // the group within the block
        lo[k] = (unsigned)__shfl((int)word, 2 * gl);
        hi[k] = (unsigned)__shfl((int)word, 2 * gl + 1);
        first_in[k] = base_in + __shfl(ahead_in, 2 * gl);
        flo[k] = (unsigned)__shfl((int)cl_lo, gl);
        fhi[k] = (unsigned)__shfl((int)cl_hi, gl);
        first_cl[k] = base_cl + __shfl(ahead_cl, gl);
        if (!c.use) flo[k] = lo[k], fhi[k] = hi[k], first_cl[k] = first_in[k];  // cloud rank = inlier rank
    }
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const unsigned long long m = ((unsigned long long)hi[k] << 32) | lo[k];
        if (!((m >> lane) & 1ull)) continue;  // (a set bit is a point below n)
        const unsigned long long mc = ((unsigned long long)fhi[k] << 32) | flo[k];
        const int rank = first_in[k] + lane_rank(lo[k], hi[k]);
        const int rank_cl = first_cl[k] + lane_rank(flo[k], fhi[k]);
        const int i = ((b * kGroupsPerChunk + wave * kGroupsPerWave + k) << 6) + lane;
        const bool st_in = rank < q.capacity;
        const bool st_cam = cam && ((mc >> lane) & 1ull) && rank_cl < q.capacity;
        if (st_in) index[rank] = i;
        if (!((st_in && lidar) || st_cam)) continue;
        float x, y, z;
        load_xyz<kStride>(q.cloud, i, x, y, z);
        if (st_in && lidar) {  // getMatrixFromIndices: the float bits of the record
            lidar[3 * (size_t)rank] = x;
            lidar[3 * (size_t)rank + 1] = y;
            lidar[3 * (size_t)rank + 2] = z;
        }
        if (st_cam) {
            const V3 pc = to_camera(c.T, (double)x, (double)y, (double)z);
            cam[3 * (size_t)rank_cl] = pc.x;
            cam[3 * (size_t)rank_cl + 1] = pc.y;
            cam[3 * (size_t)rank_cl + 2] = pc.z;
        }
    }
}

char g_error[512] = "";  // refusals without an object: mld_plane_inliers_last_error(NULL)

}  // namespace

struct mld_plane_inliers : mld_batch::Object {
    int n_seq = 0;
    int64_t max_points = 0;
    PiCalib calib{};
    CompactScratch scratch;  // the filter's ballot per group (only with the filter on); inliers and cloud points ahead of
                             // every chunk (+ the totals)
    mld_batch::DescRing<PiSeq> ring;
};

namespace {

int allocate(mld_plane_inliers* pi) {
    const int rc = pi->ring.allocate(pi, pi->n_seq);
    if (rc) return rc;
    return pi->scratch.allocate(pi, pi->n_seq, pi->max_points, kChunk, 2, pi->calib.use != 0);
}

template <int kStride>
void launch_all(mld_plane_inliers* pi, int chunks, bool any_list, mld_plane_inlier_counts* counts) {
    const unsigned S = (unsigned)pi->n_seq;
    const CompactScratch& cs = pi->scratch;
    if (chunks > 0)
        hipLaunchKernelGGL(k_pi_pass<kStride>, dim3(S, (unsigned)chunks), dim3(kBlock), 0, pi->stream, pi->ring.d_desc.get(), pi->calib,
                           cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
    hipLaunchKernelGGL(k_pi_scan, dim3(S), dim3(256), 0, pi->stream, pi->ring.d_desc.get(), (int)pi->calib.use, cs.d_cpre.get(),
                       cs.chunks_per_seq, reinterpret_cast<long long*>(counts));
    if (chunks > 0 && any_list)
        hipLaunchKernelGGL(k_pi_write<kStride>, dim3(S, (unsigned)chunks), dim3(kBlock), 0, pi->stream, pi->ring.d_desc.get(), pi->calib,
                           cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
}

}  // namespace

extern "C" {

mld_plane_inliers* mld_plane_inliers_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_params* params,
                                            const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_plane_inliers_create: n_seq must be in 1 .. 65536";
        if (max_points < 1 || max_points > kMaxPoints) return "mld_plane_inliers_create: max_points must be in 1 .. 8388607";
        if (!ctx) return "mld_plane_inliers_create: null context";
        if (!params) return "mld_plane_inliers_create: null params";
        if (!T_cam_lidar) return "mld_plane_inliers_create: null T_cam_lidar";
        return nullptr;
    };
    auto init = [&](mld_plane_inliers* pi) {
        pi->n_seq = n_seq;
        pi->max_points = max_points;
        for (int t = 0; t < 12; t++) pi->calib.T[t] = T_cam_lidar[t];
        pi->calib.thr = params->ransac_plane_treshold_camx;
        pi->calib.use = params->ransac_plane_use_camx_treshold ? 1 : 0;
        return allocate(pi);
    };
    return mld_batch::create_object<mld_plane_inliers>(g_error, "mld_plane_inliers_create", refusal(), ctx, status_out, init);
}

void mld_plane_inliers_destroy(mld_plane_inliers* pi) { mld_batch::destroy_object(pi); }

const char* mld_plane_inliers_last_error(const mld_plane_inliers* pi) { return pi ? pi->err.c_str() : g_error; }

int mld_plane_inliers_export_device(mld_plane_inliers* pi, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                                    const uint32_t* const* mask_dev, const int64_t* capacity,
                                    mld_plane_inlier_counts* counts_out_dev, int32_t* const* index_out,
                                    float* const* lidar_out, double* const* cam_out) {
    if (!pi) return no_object(g_error, "mld_plane_inliers_export_device", "pi");
#define PI_REFUSE(text) return fail(pi, MLD_ERR_INVALID_ARG, "mld_plane_inliers_export_device: " text)
    if (!pts_dev) PI_REFUSE("null table pts_dev");
    if (!n) PI_REFUSE("null table n");
    if (!mask_dev) PI_REFUSE("null table mask_dev");
    if (!capacity) PI_REFUSE("null table capacity");
    if (!counts_out_dev) PI_REFUSE("null array counts_out_dev");
    if (misaligned(counts_out_dev, 7u)) PI_REFUSE("counts_out_dev must be 8-byte aligned");
    if (!index_out) PI_REFUSE("null table index_out");
    if (stride_bytes != 16 && stride_bytes != 32) PI_REFUSE("stride_bytes must be 16 or 32");
    const int S = pi->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if (n[s] < 0) PI_REFUSE("negative n");
        if (capacity[s] < 0) PI_REFUSE("negative capacity");
        if (n[s] > pi->max_points)
            return fail(pi, MLD_ERR_CAPACITY, "mld_plane_inliers_export_device: n exceeds the max_points of the object");
        if (n[s] > 0) {
            if (!pts_dev[s]) PI_REFUSE("null array pts_dev of a sequence with points");
            if (!mask_dev[s]) PI_REFUSE("null array mask_dev of a sequence with points");
            if (misaligned(pts_dev[s], 3u)) PI_REFUSE("pts_dev must be 4-byte aligned");
            if (misaligned(mask_dev[s], 3u)) PI_REFUSE("mask_dev must be 4-byte aligned");
            if (capacity[s] > 0) {
                if (!index_out[s]) PI_REFUSE("null array index_out of a sequence with points and capacity");
                if (misaligned(index_out[s], 3u)) PI_REFUSE("index_out must be 4-byte aligned");
                if (lidar_out && lidar_out[s] && misaligned(lidar_out[s], 3u)) PI_REFUSE("lidar_out must be 4-byte aligned");
                if (cam_out && cam_out[s] && misaligned(cam_out[s], 7u)) PI_REFUSE("cam_out must be 8-byte aligned");
            }
        }
        if (n[s] > longest) longest = n[s];
    }
#undef PI_REFUSE
    bool any_list = false;
    for (int s = 0; s < S; s++) {
        PiSeq& q = pi->ring.stage[(size_t)s];
        const int64_t cap = capacity[s] < n[s] ? capacity[s] : n[s];
        q.cloud = n[s] > 0 ? static_cast<const unsigned char*>(pts_dev[s]) : nullptr;
        q.mask = n[s] > 0 ? mask_dev[s] : nullptr;
        q.index = cap > 0 ? index_out[s] : nullptr;
        q.lidar = (cap > 0 && lidar_out) ? lidar_out[s] : nullptr;
        q.cam = (cap > 0 && cam_out) ? cam_out[s] : nullptr;
        q.n = (int32_t)n[s];
        q.capacity = (int32_t)cap;
        any_list = any_list || cap > 0;
    }
    MLD_HIP(pi, hipSetDevice(pi->device));
    const int rc = pi->ring.upload(pi);
    if (rc) return rc;
    const int chunks = (int)((longest + kChunk - 1) / kChunk);  // (<= 8192)
    with_stride(stride_bytes, [&](auto stride) { launch_all<decltype(stride)::value>(pi, chunks, any_list, counts_out_dev); });
    MLD_HIP(pi, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
