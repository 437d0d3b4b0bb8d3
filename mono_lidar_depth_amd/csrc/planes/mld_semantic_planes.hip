// mld_semantic_planes.hip — SemanticPlane::CalculateInliersPlane (monolidar_fusion/src/RansacPlane.cpp:195-274) for a
// batch of sequences in one call (include/mld.h, "mld_semantic_planes").
//
// TrackletDepthModule::process builds a fresh SemanticPlane from the label image of every frame
// (tracklet_depth_module.cpp:269-284): the cloud points whose projection falls on a ground label (:198-221), a
// least-squares plane through them (:238-246), every cloud point within `inlier_threshold` of that plane (:252), the
// plane refitted to those (:253).  Here n_seq clouds are answered by four flat launches, ordered by kernel boundaries
// alone (no flags, no waiting between blocks):
//   k_sp_candidates  grid (sequence, 1024 points): projection, label lookup, moment sums per group of 64 points
//   k_sp_fit<0>      one block per sequence: first fit, n_candidates, status
//   k_sp_select      grid as the first: distance to the first plane; the ballots are the inlier mask, stored as 32-bit
//                    halves (the mask needs 4-byte alignment only); moment sums per group again
//   k_sp_fit<1>      one block per sequence: refit, the record
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; load_xyz and the smallest eigenvector of the 3x3
// covariance, shared with mld_ransac_planes: ../batch/mld_batch_device.h).  The results are nevertheless bit for bit those
// of mld_estimate_semantic_plane_device (tests/test_semantic_planes_gpu.py pins that): the helpers - plane distance,
// eigenvector, group reduction - restate that path's arithmetic, and the float moment sums keep its association:
//   the nine terms of a member (+0.0f for a non-member) over a GROUP of 64 consecutive points by the xor tree 32, 16, ..., 1;
//   the group sums, in group order, into 256 interleaved partials (group g -> partial g % 256);
//   the partials combined in index order.
// Which lane adds a pair does not matter (float addition is commutative), so the tree's steps are taken with whatever
// cross-lane move is cheapest: DPP for 8, 2 and 1, ds_swizzle for 16 and 4, a bpermute for 32.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;
constexpr int kPartials = 256;
constexpr int kGroupsPerWave = 4;    // consecutive groups a wavefront of the streaming kernels takes (loads issued up front)
constexpr int kBlockPoints = kBlock * kGroupsPerWave;  // 1024 points = 16 groups per block

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct SpSeq {
    const unsigned char* cloud;
    const uint8_t* img;
    uint32_t* mask;
    int32_t n;
    int32_t pad_;
};
static_assert(sizeof(SpSeq) == 32, "32 bytes per sequence (DESIGN.md)");

struct LabelSet {
    uint32_t w[8];  // bit l set: label l (0..255) is ground
};
struct SpCalib {
    double T[12];  // lidar -> camera, row-major 3x4
    double f, cu, cv;
};
struct SpGeom {
    int32_t rows, cols, stride;
};
struct GroupSums {
    float s[9];  // xx, xy, xz, yy, yz, zz, x, y, z of the group's members
    int count;   // members
};
static_assert(sizeof(GroupSums) == 40, "40 bytes of scratch per 64 points");
static_assert(sizeof(mld_semantic_plane_result) == 32, "mld.h");

__device__ __forceinline__ float plane_dist(const float c[4], float x, float y, float z) {
    return fabsf(c[0] * x + c[1] * y + c[2] * z + c[3]);
}

// x of the lane whose number differs in bit K.  Every lane of the wavefront must be active.
template <int K>
__device__ __forceinline__ float lane_xor(float x) {
    const int v = __float_as_int(x);
    if constexpr (K == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));        // quad_perm 1,0,3,2
    else if constexpr (K == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));   // quad_perm 2,3,0,1
    else if constexpr (K == 8) return __int_as_float(__builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false));  // row_ror 8
    else if constexpr (K == 4) return __int_as_float(__builtin_amdgcn_ds_swizzle(v, 0x101F));                     // xor 4 in 32
    else if constexpr (K == 16) return __int_as_float(__builtin_amdgcn_ds_swizzle(v, 0x401F));                    // xor 16 in 32
    else return __shfl_xor(x, 32);
}

template <int K>
__device__ __forceinline__ void tree_step(float (&a)[9]) {
#pragma unroll
    for (int t = 0; t < 9; t++) a[t] = a[t] + lane_xor<K>(a[t]);
}

// The nine terms of a member (zeros for a non-member) reduced over the wavefront's 64 points; lane 0 stores them.
__device__ __forceinline__ void group_reduce(bool member, float x, float y, float z, GroupSums* __restrict__ out, int lane) {
    float a[9];
    a[0] = member ? x * x : 0.0f;
    a[1] = member ? x * y : 0.0f;
    a[2] = member ? x * z : 0.0f;
    a[3] = member ? y * y : 0.0f;
    a[4] = member ? y * z : 0.0f;
    a[5] = member ? z * z : 0.0f;
    a[6] = member ? x : 0.0f;
    a[7] = member ? y : 0.0f;
    a[8] = member ? z : 0.0f;
    tree_step<32>(a);
    tree_step<16>(a);
    tree_step<8>(a);
    tree_step<4>(a);
    tree_step<2>(a);
    tree_step<1>(a);
    const int cnt = (int)__popcll(__ballot(member));
    if (lane == 0) {
        MLD_BATCH_GLOBAL float* o = as_global(out->s);
#pragma unroll
        for (int t = 0; t < 9; t++) o[t] = a[t];
        *as_global(&out->count) = cnt;
    }
}

// :198-221  pcl::transformPointCloud (double arithmetic, float result), project() (K * p as Eigen evaluates a
// 3x3 * 3x1 product: x0 + (x1 + x2); p /= p[2]; cv::Point truncation), image bounds, label lookup.  The pixels
// x == cols / y == rows the reference reads out of bounds count as unlabeled; non-finite projections as invalid.
__device__ __forceinline__ bool is_candidate(float fx, float fy, float fz, const SpCalib& sc, const uint8_t* __restrict__ img,
                                             const SpGeom& g, const LabelSet& ls) {
    const double x = fx, y = fy, z = fz;
    const float xc = (float)(((sc.T[0] * x + sc.T[1] * y) + sc.T[2] * z) + sc.T[3]);
    const float yc = (float)(((sc.T[4] * x + sc.T[5] * y) + sc.T[6] * z) + sc.T[7]);
    const float zc = (float)(((sc.T[8] * x + sc.T[9] * y) + sc.T[10] * z) + sc.T[11]);
    const double px = (double)xc, py = (double)yc, pz = (double)zc;
    const double p0 = sc.f * px + (0.0 * py + sc.cu * pz);
    const double p1 = 0.0 * px + (sc.f * py + sc.cv * pz);
    const double p2 = 0.0 * px + (0.0 * py + 1.0 * pz);
    const double u = p0 / p2, v = p1 / p2;
    bool flag = false;
    if (isfinite(u) && isfinite(v) && fabs(u) < 2147483648.0 && fabs(v) < 2147483648.0) {
        const int ix = (int)u, iy = (int)v;
        if (ix >= 0 && ix < g.cols && iy >= 0 && iy < g.rows) {
            const unsigned l = as_global(img)[(size_t)iy * (size_t)g.stride + (size_t)ix];
            flag = (ls.w[l >> 5] >> (l & 31)) & 1u;
        }
    }
    return flag;
}

// Grid (sequence, block of 1024 points).  Wavefront w of block b takes the groups 16 b + 4 w + k, k = 0..3.
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_sp_candidates(const SpSeq* __restrict__ desc, SpCalib sc, SpGeom g, LabelSet ls,
                                                         GroupSums* __restrict__ gs_all, long long groups_per_seq) {
    const SpSeq q = desc[blockIdx.x];
    const int n = q.n;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int first = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave * kWave;  // the wavefront's first point
    if (first >= n) return;  // (uniform in the wavefront; max_points < 2^23: no overflow)
    GroupSums* __restrict__ gs = gs_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    float x[kGroupsPerWave], y[kGroupsPerWave], z[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        x[k] = y[k] = z[k] = 0.f;
        if (i < n) load_xyz<kStride>(q.cloud, i, x[k], y[k], z[k]);
    }
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave;
        if (i0 >= n) break;  // (uniform)
        const bool flag = (i0 + lane < n) && is_candidate(x[k], y[k], z[k], sc, q.img, g, ls);
        group_reduce(flag, x[k], y[k], z[k], gs + (i0 >> 6), lane);
    }
}

// SampleConsensusModelPlane::selectWithinDistance over the whole cloud (:252), float distance < double threshold, against
// the first plane of the sequence.  A sequence whose first fit failed (status 1) gets a mask of zeros and reads no cloud.
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_sp_select(const SpSeq* __restrict__ desc, const float* __restrict__ first_plane,
                                                     const mld_semantic_plane_result* __restrict__ res, double thr,
                                                     GroupSums* __restrict__ gs_all, long long groups_per_seq) {
    const SpSeq q = desc[blockIdx.x];
    const int n = q.n;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int first = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave * kWave;
    if (first >= n) return;
    const bool live = res[blockIdx.x].status == 0;
    const float* cp = first_plane + 4 * (size_t)blockIdx.x;
    const float c[4] = {cp[0], cp[1], cp[2], cp[3]};
    GroupSums* __restrict__ gs = gs_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    const int words = (n + 31) >> 5;
    float x[kGroupsPerWave], y[kGroupsPerWave], z[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        x[k] = y[k] = z[k] = 0.f;
        if (live && i < n) load_xyz<kStride>(q.cloud, i, x[k], y[k], z[k]);
    }
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave;
        if (i0 >= n) break;  // (uniform)
        const bool flag = live && (i0 + lane < n) && ((double)plane_dist(c, x[k], y[k], z[k]) < thr);
        const unsigned long long m = __ballot(flag);
        // the two halves of the ballot by the lanes 0 and 32; the second half only where the mask has that word
        const int w = (i0 >> 5) + (lane >> 5);
        if ((lane & 31) == 0 && w < words) as_global(q.mask)[w] = (uint32_t)(lane ? (m >> 32) : m);
        if (live) group_reduce(flag, x[k], y[k], z[k], gs + (i0 >> 6), lane);
    }
}

// optimizeModelCoefficients from the group sums of one sequence: fewer than 4 members return the fallback.  One block of
// 256 threads per sequence.
//   kStage 0: the candidates' fit; fallback = the dummy prior (0, 0, 1, 0) (:241-242).  Writes n_candidates, status
//             (fewer than 3 candidates = ExceptionPclInvalid, :224-227) and the first plane.
//   kStage 1: the refit on the selected points; fallback = the first plane.  Writes the rest of the record.
template <int kStage>
__global__ __launch_bounds__(kPartials) void k_sp_fit(const SpSeq* __restrict__ desc, const GroupSums* __restrict__ gs_all,
                                                     long long groups_per_seq, float* __restrict__ first_plane,
                                                     mld_semantic_plane_result* __restrict__ res) {
    __shared__ float acc[kPartials][9];
    __shared__ float s9s[9];
    __shared__ int wcnt[kPartials / kWave];
    const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
    mld_semantic_plane_result* r = res + s;
    float* fp = first_plane + 4 * (size_t)s;
    if (kStage == 1 && r->status != 0) {  // (uniform in the block)
        if (tid == 0) {
            r->coeffs[0] = r->coeffs[1] = r->coeffs[2] = r->coeffs[3] = 0.0f;
            r->n_inliers = 0;
            r->reserved = 0;
        }
        return;
    }
    const int G = (desc[s].n + kWave - 1) / kWave;
    const GroupSums* __restrict__ gs = gs_all + (size_t)s * (size_t)groups_per_seq;
    float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cnt = 0;
    for (int g = tid; g < G; g += kPartials) {
        const GroupSums q = gs[g];
#pragma unroll
        for (int t = 0; t < 9; t++) a[t] += q.s[t];
        cnt += q.count;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & (kWave - 1)) == 0) wcnt[tid / kWave] = cnt;
    for (int t = 0; t < 9; t++) acc[tid][t] = a[t];
    __syncthreads();
    int m = 0;
    for (int q = 0; q < kPartials / kWave; q++) m += wcnt[q];
    // the 256 partials of each sum combined in index order, by nine lanes side by side
    if (tid < 9) {
        float sum = 0.0f;
#pragma unroll 16
        for (int p = 0; p < kPartials; p++) sum += acc[p][tid];
        s9s[tid] = sum / (float)m;
    }
    __syncthreads();
    if (tid != 0) return;
    float c4[4] = {0.f, 0.f, 1.f, 0.f};
    if (kStage == 1)
        for (int t = 0; t < 4; t++) c4[t] = fp[t];
    if (m >= 4) {
        float s9[9];
        for (int t = 0; t < 9; t++) s9[t] = s9s[t];
        const float cov[6] = {s9[0] - s9[6] * s9[6], s9[1] - s9[6] * s9[7], s9[2] - s9[6] * s9[8],
                              s9[3] - s9[7] * s9[7], s9[4] - s9[7] * s9[8], s9[5] - s9[8] * s9[8]};
        double sd[6] = {cov[0], cov[1], cov[2], cov[3], cov[4], cov[5]}, n0[3];
        smallest_eigvec(sd, n0);
        const float e0 = (float)n0[0], e1 = (float)n0[1], e2 = (float)n0[2];
        c4[0] = e0;
        c4[1] = e1;
        c4[2] = e2;
        c4[3] = -1.0f * (e0 * s9[6] + e1 * s9[7] + e2 * s9[8]);
    }
    if (kStage == 0) {
        for (int t = 0; t < 4; t++) fp[t] = c4[t];
        r->n_candidates = m;
        r->status = m < 3 ? 1 : 0;
    } else {
        for (int t = 0; t < 4; t++) r->coeffs[t] = c4[t];
        r->n_inliers = m;
        r->reserved = 0;
    }
}

char g_error[512] = "";  // refusals without an object: mld_semantic_planes_last_error(NULL)

}  // namespace

struct mld_semantic_planes : mld_batch::Object {
    int n_seq = 0;
    int64_t max_points = 0;
    long long groups_per_seq = 0;
    SpCalib calib{};
    mld_batch::DeviceBuffer<GroupSums> d_groups;
    mld_batch::DeviceBuffer<float> d_first;  // the first plane of every sequence
    mld_batch::DescRing<SpSeq> ring;
};

namespace {

int allocate(mld_semantic_planes* sp) {
    int rc;
    if ((rc = sp->ring.allocate(sp, sp->n_seq))) return rc;
    if ((rc = sp->d_groups.allocate(sp, (size_t)sp->n_seq * (size_t)sp->groups_per_seq))) return rc;
    return sp->d_first.allocate(sp, (size_t)sp->n_seq * 4);
}

template <int kStride>
void launch_all(mld_semantic_planes* sp, int chunks, const SpGeom& g, const LabelSet& ls, double thr,
                mld_semantic_plane_result* res) {
    const int S = sp->n_seq;
    const dim3 stream_grid((unsigned)S, (unsigned)chunks), fit_grid((unsigned)S);
    if (chunks > 0)
        hipLaunchKernelGGL(k_sp_candidates<kStride>, stream_grid, dim3(kBlock), 0, sp->stream, sp->ring.d_desc.get(), sp->calib, g, ls,
                           sp->d_groups.get(), sp->groups_per_seq);
    hipLaunchKernelGGL(k_sp_fit<0>, fit_grid, dim3(kPartials), 0, sp->stream, sp->ring.d_desc.get(), sp->d_groups.get(), sp->groups_per_seq,
                       sp->d_first.get(), res);
    if (chunks > 0)
        hipLaunchKernelGGL(k_sp_select<kStride>, stream_grid, dim3(kBlock), 0, sp->stream, sp->ring.d_desc.get(), sp->d_first.get(), res, thr,
                           sp->d_groups.get(), sp->groups_per_seq);
    hipLaunchKernelGGL(k_sp_fit<1>, fit_grid, dim3(kPartials), 0, sp->stream, sp->ring.d_desc.get(), sp->d_groups.get(), sp->groups_per_seq,
                       sp->d_first.get(), res);
}

}  // namespace

extern "C" {

mld_semantic_planes* mld_semantic_planes_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_camera* camera,
                                                const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_semantic_planes_create: n_seq must be in 1 .. 65536";
        if (max_points < 1 || max_points > kMaxPoints) return "mld_semantic_planes_create: max_points must be in 1 .. 8388607";
        if (!ctx) return "mld_semantic_planes_create: null context";
        if (!camera) return "mld_semantic_planes_create: null camera";
        if (!T_cam_lidar) return "mld_semantic_planes_create: null T_cam_lidar";
        return nullptr;
    };
    auto init = [&](mld_semantic_planes* sp) {
        sp->n_seq = n_seq;
        sp->max_points = max_points;
        sp->groups_per_seq = (long long)((max_points + kWave - 1) / kWave);
        for (int t = 0; t < 12; t++) sp->calib.T[t] = T_cam_lidar[t];
        sp->calib.f = camera->focal_length;
        sp->calib.cu = camera->principal_point_x;
        sp->calib.cv = camera->principal_point_y;
        return allocate(sp);
    };
    return mld_batch::create_object<mld_semantic_planes>(g_error, "mld_semantic_planes_create", refusal(), ctx, status_out, init);
}

void mld_semantic_planes_destroy(mld_semantic_planes* sp) { mld_batch::destroy_object(sp); }

const char* mld_semantic_planes_last_error(const mld_semantic_planes* sp) { return sp ? sp->err.c_str() : g_error; }

int mld_semantic_planes_estimate_device(mld_semantic_planes* sp, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                                        const uint8_t* const* label_image_dev, int rows, int cols, int row_stride_bytes,
                                        const int32_t* ground_labels, int n_labels, double inlier_threshold,
                                        mld_semantic_plane_result* result_out_dev, uint32_t* const* mask_out_dev) {
    if (!sp) return no_object(g_error, "mld_semantic_planes_estimate_device", "sp");
#define SP_REFUSE(text) return fail(sp, MLD_ERR_INVALID_ARG, "mld_semantic_planes_estimate_device: " text)
    if (!pts_dev) SP_REFUSE("null table pts_dev");
    if (!n) SP_REFUSE("null table n");
    if (!label_image_dev) SP_REFUSE("null table label_image_dev");
    if (!result_out_dev) SP_REFUSE("null array result_out_dev");
    if (!mask_out_dev) SP_REFUSE("null table mask_out_dev");
    if (stride_bytes != 16 && stride_bytes != 32) SP_REFUSE("stride_bytes must be 16 or 32");
    if (rows < 1 || cols < 1) SP_REFUSE("rows and cols must be >= 1");
    if (row_stride_bytes < cols) SP_REFUSE("row_stride_bytes must be >= cols");
    if (n_labels < 0) SP_REFUSE("n_labels must be >= 0");
    if (n_labels > 0 && !ground_labels) SP_REFUSE("null ground_labels with n_labels > 0");
    const int S = sp->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if (n[s] < 0) SP_REFUSE("negative n");
        if (n[s] > sp->max_points)
            return fail(sp, MLD_ERR_CAPACITY, "mld_semantic_planes_estimate_device: n exceeds the max_points of the object");
        if (n[s] > 0) {
            if (!pts_dev[s]) SP_REFUSE("null array pts_dev of a sequence with points");
            if (!label_image_dev[s]) SP_REFUSE("null array label_image_dev of a sequence with points");
            if (!mask_out_dev[s]) SP_REFUSE("null array mask_out_dev of a sequence with points");
            if (misaligned(pts_dev[s], 3u) || misaligned(mask_out_dev[s], 3u))
                SP_REFUSE("pts_dev and mask_out_dev must be 4-byte aligned");
        }
        if (n[s] > longest) longest = n[s];
    }
#undef SP_REFUSE
    for (int s = 0; s < S; s++) {
        SpSeq& q = sp->ring.stage[(size_t)s];
        q.cloud = static_cast<const unsigned char*>(pts_dev[s]);
        q.img = label_image_dev[s];
        q.mask = mask_out_dev[s];
        q.n = (int32_t)n[s];
        q.pad_ = 0;
    }
    LabelSet ls{};
    for (int i = 0; i < n_labels; i++)
        if (ground_labels[i] >= 0 && ground_labels[i] < 256) ls.w[ground_labels[i] >> 5] |= 1u << (ground_labels[i] & 31);
    MLD_HIP(sp, hipSetDevice(sp->device));
    const int rc = sp->ring.upload(sp);
    if (rc) return rc;
    const SpGeom g{rows, cols, row_stride_bytes};
    const int chunks = (int)((longest + kBlockPoints - 1) / kBlockPoints);  // (<= 8192)
    with_stride(stride_bytes,
                [&](auto stride) { launch_all<decltype(stride)::value>(sp, chunks, g, ls, inlier_threshold, result_out_dev); });
    MLD_HIP(sp, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
