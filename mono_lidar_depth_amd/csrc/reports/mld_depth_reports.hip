// mld_depth_reports.hip — the two per-frame products of the reference's ROS node that the batched layer lacked, for a batch
// of sequences in one call (include/mld.h, "mld_depth_reports"): the depth-calculation statistics (getDepthCalcStats,
// filled by LogDepthCalcStats, DepthEstimator.cpp:1039-1090, published by PublishDepthCalcStats) and the interpolated
// cloud (getCloudInterpolated, published by PublishPointCloudInterpolated) - the intersection point of the viewing ray
// with the local plane for every feature with depth >= 0, in feature order.  Features, depths and types are read where
// they lie, nothing is allocated per call and nothing comes back to the host.
//
// Up to three launches, ordered by kernel boundaries alone (no global atomics, no memset, no flags between blocks):
//   k_dr_pass   grid (sequence, 1024 features): depth and type, both coalesced; the validity ballot as one 64-bit word per
//               64 features, the chunk's valid count and its 22-bin type histogram (21 types + other, built in LDS), all in
//               the object's device scratch
//   k_dr_scan   one block per sequence: exclusive prefix of the chunk counts, in place; the sum of the chunk histograms; the
//               whole 192-byte record
//   k_dr_write  (only when points are asked for) grid as the pass: rank of a valid feature = chunk base + popcounts of the
//               chunk's earlier words + prefix within its word.  Only the valid lanes below the capacity load u, v and d
//               again and store the point and, where asked for, the feature index.
// One templated body serves both entry points; only the loader differs: LoadF64 reads the interleaved f64 (u, v) and f64
// depths of mld_calculate_depths_device, LoadF32 the split f32 u / v / depth of the tracklet layer, u and v truncated to
// the integer pixel that layer evaluates.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring, object skeleton and compaction scratch: ../batch/mld_batch_object.h; the compaction's device
// pieces: ../batch/mld_batch_device.h).  The point is the arithmetic of the host shim's
// getCloudInterpolated, operation for operation in f64, and this unit is compiled without contraction like the rest of
// the library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;
constexpr int kGroupsPerWave = 4;                // consecutive groups of 64 features a wavefront takes
constexpr int kChunk = kBlock * kGroupsPerWave;  // 1024 features = 16 groups per block
constexpr int kGroupsPerChunk = kChunk / kWave;
constexpr int kBins = MLD_RESULT_TYPE_COUNT + 1;  // 21 types + other
constexpr int kScanRows = 256 / kBins;            // rows of kBins threads that sum the chunk histograms (11)

static_assert(sizeof(mld_depth_report) == 192 && sizeof(mld_depth_report) == 8 * (kBins + 2), "24 int64 (include/mld.h)");

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct DrSeq {
    const void* a;        // LoadF64: uv, 2 x n f64 interleaved; LoadF32: u, n f32
    const void* b;        // LoadF32: v, n f32
    const void* depth;    // n f64 / f32
    const int32_t* type;  // n, or null: counts and other are 0
    double* points;       // 3 x capacity, null: capacity 0
    int32_t* feature;     // capacity, or null
    int32_t n;
    int32_t capacity;  // min(capacity[s], n[s]): a rank is below n; 0 without points_out
};
static_assert(sizeof(DrSeq) == 56, "56 bytes per sequence (DESIGN.md)");

struct DrCam {
    double f, cu, cv;
};

// (u, v) of a feature as ONE load, with the 8-byte alignment the C-ABI asks for (gfx950 takes multi-dword global loads at
// any dword address).
typedef double double2v __attribute__((ext_vector_type(2)));
typedef double2v double2u __attribute__((aligned(8)));

// DepthEstimator layer: uv as 2 x F f64 column-major, depth f64 (mld_calculate_depths_device).
struct LoadF64 {
    static constexpr bool kF64 = true;
    static __device__ __forceinline__ double depth(const DrSeq& q, int i) {
        return as_global(static_cast<const double*>(q.depth))[i];
    }
    static __device__ __forceinline__ void uv(const DrSeq& q, int i, double& u, double& v) {
        const double2v r = *(const MLD_BATCH_GLOBAL double2u*)(static_cast<const double*>(q.a) + 2 * (size_t)i);
        u = r.x, v = r.y;
    }
};

// Tracklet layer: u, v, depth as f32 arrays (mld_tracklets_depths_device / mld_tracklets_step_device).  truncf is the
// integer pixel that layer evaluates (std::pair<int,int>), defined for NaN, inf and values beyond int as well.
struct LoadF32 {
    static constexpr bool kF64 = false;
    static __device__ __forceinline__ double depth(const DrSeq& q, int i) {
        return (double)as_global(static_cast<const float*>(q.depth))[i];
    }
    static __device__ __forceinline__ void uv(const DrSeq& q, int i, double& u, double& v) {
        u = (double)truncf(as_global(static_cast<const float*>(q.a))[i]);
        v = (double)truncf(as_global(static_cast<const float*>(q.b))[i]);
    }
};

// Grid (sequence, chunk of 1024 features).  gm: one 64-bit validity mask per 64 features; cpre[c + 1]: the valid features
// of chunk c (k_dr_scan makes them a prefix); hist: kBins counts per chunk (written only where the sequence has types).
template <typename Load>
__global__ __launch_bounds__(kBlock) void k_dr_pass(const DrSeq* __restrict__ desc, unsigned long long* __restrict__ gm_all,
                                                   long long groups_per_seq, int* __restrict__ cpre_all,
                                                   int* __restrict__ hist_all, long long chunks_per_seq) {
    __shared__ int wsum[kBlock / kWave];
    __shared__ int bins[kBins];
    const DrSeq q = desc[blockIdx.x];
    const int n = q.n;
    if ((long long)blockIdx.y * kChunk >= (long long)n) return;  // (uniform in the block)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int first = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave * kWave;  // the wavefront's first feature
    unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    MLD_BATCH_GLOBAL const int32_t* type = as_global(q.type);
    double d[kGroupsPerWave];
    int t[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        d[k] = -1.;
        t[k] = 0;
        if (i < n) {
            d[k] = Load::depth(q, i);
            if (type) t[k] = type[i];
        }
    }
    if (type) {  // (uniform in the block)
        if (threadIdx.x < kBins) bins[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kGroupsPerWave; k++) {
            const int i = first + k * kWave + lane;
            // (one LDS add per feature.  A loop over the bins that occur in the group - one add per bin, by its first lane -
            //  made the pass slower, 14.0 against 8.7 us on 256 x 10 000 tracks: profiles/depth_reports.md)
            if (i < n) atomicAdd(&bins[(t[k] >= 0 && t[k] < MLD_RESULT_TYPE_COUNT) ? t[k] : MLD_RESULT_TYPE_COUNT], 1);
        }
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave;
        const unsigned long long m = __ballot((i0 + lane < n) && (d[k] >= 0.));  // NaN is out; -0.0 and +inf are in
        if (lane == 0 && i0 < n) *as_global(gm + (i0 >> 6)) = m;
        cnt += (int)__popcll(m);
    }
    if (lane == 0) wsum[wave] = cnt;
    chunk_count(wsum, cpre_all, chunks_per_seq);
    if (type && threadIdx.x < kBins)
        *as_global(hist_all + ((size_t)blockIdx.x * (size_t)chunks_per_seq + blockIdx.y) * kBins + threadIdx.x) = bins[threadIdx.x];
}

// One block per sequence.  Exclusive prefix over the chunk counts, in place: cpre[c] = valid features ahead of chunk c (the
// loop carries the sum over any number of chunks, up to 16384); then the chunk histograms summed per bin by kScanRows rows
// of kBins threads; then the record, all 24 words of it.
__global__ __launch_bounds__(256) void k_dr_scan(const DrSeq* __restrict__ desc, int* __restrict__ cpre_all,
                                                const int* __restrict__ hist_all, long long chunks_per_seq,
                                                long long* __restrict__ report) {
    __shared__ long long part[kScanRows][kBins];
    const int n = desc[blockIdx.x].n;
    const bool typed = desc[blockIdx.x].type != nullptr;
    const int NC = (int)(((long long)n + kChunk - 1) / kChunk);
    const int tid = (int)threadIdx.x;
    const int carry = scan_chunk_counts(cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1), NC);
    const int row = tid / kBins, bin = tid - row * kBins;
    if (row < kScanRows) {
        long long sum = 0;
        if (typed) {
            const int* __restrict__ hist = hist_all + (size_t)blockIdx.x * (size_t)chunks_per_seq * kBins;
            for (int c = row; c < NC; c += kScanRows) sum += (long long)hist[(size_t)c * kBins + bin];
        }
        part[row][bin] = sum;
    }
    __syncthreads();
    if (tid < kBins + 2) {
        long long word;
        if (tid < kBins) {  // counts[0 .. 20], other
            word = 0;
#pragma unroll
            for (int r = 0; r < kScanRows; r++) word += part[r][tid];
        } else {
            word = tid == kBins ? (long long)n : (long long)carry;  // point_count, n_interpolated
        }
        *as_global(report + (size_t)blockIdx.x * (kBins + 2) + tid) = word;
    }
}

// Grid as the pass.  Every wavefront reads the (up to 16) masks of its block, one per lane, and scans their counts; the
// valid lanes of its four groups whose rank is below the capacity then do the work.
template <typename Load>
__global__ __launch_bounds__(kBlock) void k_dr_write(const DrSeq* __restrict__ desc, DrCam c,
                                                    const unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                    const int* __restrict__ cpre_all, long long chunks_per_seq) {
    const DrSeq q = desc[blockIdx.x];
    const int n = q.n;
    const int b = (int)blockIdx.y;
    if ((long long)b * kChunk >= (long long)n) return;  // (uniform in the block)
    const int* __restrict__ cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1);
    const int base = cpre[b];
    if (base >= q.capacity || cpre[b + 1] == base) return;  // nothing of this chunk is stored (uniform in the block)
    const unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int G = (int)(((long long)n + kWave - 1) / kWave);
    const int g_mine = b * kGroupsPerChunk + lane;  // lanes 0..15: the masks of the block
    const unsigned long long mine = (lane < kGroupsPerChunk && g_mine < G) ? gm[g_mine] : 0ull;
    MLD_BATCH_GLOBAL double* points = as_global(q.points);
    MLD_BATCH_GLOBAL int32_t* feature = as_global(q.feature);
    // (the cross-lane reads while every lane is here)
    unsigned lo[kGroupsPerWave], hi[kGroupsPerWave];
    int first_rank[kGroupsPerWave];
    group_ranks<kGroupsPerChunk>(mine, base, lane, wave, lo, hi, first_rank);
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const unsigned long long m = ((unsigned long long)hi[k] << 32) | lo[k];
        if (!((m >> lane) & 1ull)) continue;  // (a set bit is a feature below n)
        const int rank = first_rank[k] + lane_rank(lo[k], hi[k]);
        if (rank >= q.capacity) continue;
        const int i = ((b * kGroupsPerChunk + wave * kGroupsPerWave + k) << 6) + lane;
        double u, v;
        Load::uv(q, i, u, v);
        const double d = Load::depth(q, i);
        // host/monolidar_fusion/DepthEstimator.h getCloudInterpolated: (u - cu) / f * d, (v - cv) / f * d, d
        points[3 * (size_t)rank] = (u - c.cu) / c.f * d;
        points[3 * (size_t)rank + 1] = (v - c.cv) / c.f * d;
        points[3 * (size_t)rank + 2] = d;
        if (feature) feature[rank] = i;
    }
}

char g_error[512] = "";  // refusals without an object: mld_depth_reports_last_error(NULL)

}  // namespace

struct mld_depth_reports : mld_batch::Object {
    int n_seq = 0;
    int64_t max_features = 0;
    DrCam cam{};
    CompactScratch scratch;  // validity mask per group; valid features ahead of every chunk (+ the total)
    mld_batch::DeviceBuffer<int> d_hist;  // kBins counts per chunk
    mld_batch::DescRing<DrSeq> ring;
};

namespace {

int allocate(mld_depth_reports* dr) {
    int rc;
    if ((rc = dr->ring.allocate(dr, dr->n_seq))) return rc;
    if ((rc = dr->scratch.allocate(dr, dr->n_seq, dr->max_features, kChunk, 1))) return rc;
    return dr->d_hist.allocate(dr, (size_t)dr->n_seq * (size_t)dr->scratch.chunks_per_seq * kBins);
}

// The shared body of the two entry points.  a / b: the coordinate tables (LoadF64: uv and none; LoadF32: u and v).
template <typename Load>
int collect(mld_depth_reports* dr, const char* fn, const char* a_name, const void* const* a, const void* const* b,
            const void* const* depth, const int32_t* const* type, const int64_t* n_features, const int64_t* capacity,
            mld_depth_report* report_out_dev, double* const* points_out, int32_t* const* feature_out) {
    constexpr bool kF64 = Load::kF64;
    constexpr unsigned in_mask = kF64 ? 7u : 3u;
    auto refuse = [&](int code, const char* text) {
        dr->err = std::string(fn) + ": " + text;
        return code;
    };
    if (!a) return refuse(MLD_ERR_INVALID_ARG, (std::string("null table ") + a_name).c_str());
    if (!kF64 && !b) return refuse(MLD_ERR_INVALID_ARG, "null table v");
    if (!depth) return refuse(MLD_ERR_INVALID_ARG, "null table depth");
    if (!n_features) return refuse(MLD_ERR_INVALID_ARG, "null table n_features");
    if (!report_out_dev) return refuse(MLD_ERR_INVALID_ARG, "null array report_out_dev");
    if (misaligned(report_out_dev, 7u)) return refuse(MLD_ERR_INVALID_ARG, "report_out_dev must be 8-byte aligned");
    if (points_out && !capacity) return refuse(MLD_ERR_INVALID_ARG, "null table capacity with points_out");
    const int S = dr->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        const int64_t n = n_features[s];
        if (n < 0) return refuse(MLD_ERR_INVALID_ARG, "negative n_features");
        if (n > dr->max_features) return refuse(MLD_ERR_CAPACITY, "n_features exceeds the max_features of the object");
        if (points_out && capacity[s] < 0) return refuse(MLD_ERR_INVALID_ARG, "negative capacity");
        if (n > 0) {
            if (!a[s]) return refuse(MLD_ERR_INVALID_ARG, (std::string("null array ") + a_name + " of a sequence with features").c_str());
            if (!kF64 && !b[s]) return refuse(MLD_ERR_INVALID_ARG, "null array v of a sequence with features");
            if (!depth[s]) return refuse(MLD_ERR_INVALID_ARG, "null array depth of a sequence with features");
            if (misaligned(a[s], in_mask))
                return refuse(MLD_ERR_INVALID_ARG, (std::string(a_name) + (kF64 ? " must be 8-byte aligned" : " must be 4-byte aligned")).c_str());
            if (!kF64 && misaligned(b[s], 3u)) return refuse(MLD_ERR_INVALID_ARG, "v must be 4-byte aligned");
            if (misaligned(depth[s], in_mask))
                return refuse(MLD_ERR_INVALID_ARG, kF64 ? "depth must be 8-byte aligned" : "depth must be 4-byte aligned");
            if (type && type[s] && misaligned(type[s], 3u)) return refuse(MLD_ERR_INVALID_ARG, "type must be 4-byte aligned");
            if (points_out && capacity[s] > 0) {
                if (!points_out[s]) return refuse(MLD_ERR_INVALID_ARG, "null array points_out of a sequence with features and capacity");
                if (misaligned(points_out[s], 7u)) return refuse(MLD_ERR_INVALID_ARG, "points_out must be 8-byte aligned");
                if (feature_out && feature_out[s] && misaligned(feature_out[s], 3u))
                    return refuse(MLD_ERR_INVALID_ARG, "feature_out must be 4-byte aligned");
            }
        }
        if (n > longest) longest = n;
    }
    bool any_points = false;
    for (int s = 0; s < S; s++) {
        DrSeq& q = dr->ring.stage[(size_t)s];
        const int64_t n = n_features[s];
        const int64_t cap = !points_out ? 0 : (capacity[s] < n ? capacity[s] : n);
        q.a = n > 0 ? a[s] : nullptr;
        q.b = (n > 0 && b) ? b[s] : nullptr;
        q.depth = n > 0 ? depth[s] : nullptr;
        q.type = (n > 0 && type) ? type[s] : nullptr;
        q.points = cap > 0 ? points_out[s] : nullptr;
        q.feature = (cap > 0 && feature_out) ? feature_out[s] : nullptr;
        q.n = (int32_t)n;
        q.capacity = (int32_t)cap;
        any_points = any_points || cap > 0;
    }
    MLD_HIP(dr, hipSetDevice(dr->device));
    const int rc = dr->ring.upload(dr);
    if (rc) return rc;
    const unsigned chunks = (unsigned)((longest + kChunk - 1) / kChunk);  // (<= 16384)
    const unsigned Su = (unsigned)S;
    const CompactScratch& cs = dr->scratch;
    if (chunks > 0)
        hipLaunchKernelGGL(k_dr_pass<Load>, dim3(Su, chunks), dim3(kBlock), 0, dr->stream, dr->ring.d_desc.get(), cs.d_gm.get(),
                           cs.groups_per_seq, cs.d_cpre.get(), dr->d_hist.get(), cs.chunks_per_seq);
    hipLaunchKernelGGL(k_dr_scan, dim3(Su), dim3(256), 0, dr->stream, dr->ring.d_desc.get(), cs.d_cpre.get(), dr->d_hist.get(), cs.chunks_per_seq,
                       reinterpret_cast<long long*>(report_out_dev));
    if (chunks > 0 && any_points)
        hipLaunchKernelGGL(k_dr_write<Load>, dim3(Su, chunks), dim3(kBlock), 0, dr->stream, dr->ring.d_desc.get(), dr->cam, cs.d_gm.get(),
                           cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
    MLD_HIP(dr, hipGetLastError());
    return MLD_OK;
}

}  // namespace

extern "C" {

mld_depth_reports* mld_depth_reports_create(mld_ctx* ctx, int n_seq, int64_t max_features, const mld_camera* camera,
                                            int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_depth_reports_create: n_seq must be in 1 .. 65536";
        if (max_features < 1 || max_features > kMaxFeatures) return "mld_depth_reports_create: max_features must be in 1 .. 16777216";
        if (!ctx) return "mld_depth_reports_create: null context";
        if (!camera) return "mld_depth_reports_create: null camera";
        if (!std::isfinite(camera->focal_length) || camera->focal_length == 0.)
            return "mld_depth_reports_create: camera focal_length must be finite and not 0";
        return nullptr;
    };
    auto init = [&](mld_depth_reports* dr) {
        dr->n_seq = n_seq;
        dr->max_features = max_features;
        dr->cam.f = camera->focal_length;
        dr->cam.cu = camera->principal_point_x;
        dr->cam.cv = camera->principal_point_y;
        return allocate(dr);
    };
    return mld_batch::create_object<mld_depth_reports>(g_error, "mld_depth_reports_create", refusal(), ctx, status_out, init);
}

void mld_depth_reports_destroy(mld_depth_reports* dr) { mld_batch::destroy_object(dr); }

const char* mld_depth_reports_last_error(const mld_depth_reports* dr) { return dr ? dr->err.c_str() : g_error; }

int mld_depth_reports_collect_device(mld_depth_reports* dr, const double* const* uv, const double* const* depth,
                                     const int32_t* const* type, const int64_t* n_features, const int64_t* capacity,
                                     mld_depth_report* report_out_dev, double* const* points_out, int32_t* const* feature_out) {
    if (!dr) return no_object(g_error, "mld_depth_reports_collect_device", "dr");
    return collect<LoadF64>(dr, "mld_depth_reports_collect_device", "uv", reinterpret_cast<const void* const*>(uv), nullptr,
                            reinterpret_cast<const void* const*>(depth), type, n_features, capacity, report_out_dev, points_out,
                            feature_out);
}

int mld_depth_reports_collect_tracks_device(mld_depth_reports* dr, const float* const* u, const float* const* v,
                                            const float* const* depth, const int32_t* const* type, const int64_t* n_features,
                                            const int64_t* capacity, mld_depth_report* report_out_dev, double* const* points_out,
                                            int32_t* const* feature_out) {
    if (!dr) return no_object(g_error, "mld_depth_reports_collect_tracks_device", "dr");
    return collect<LoadF32>(dr, "mld_depth_reports_collect_tracks_device", "u", reinterpret_cast<const void* const*>(u),
                            reinterpret_cast<const void* const*>(v), reinterpret_cast<const void* const*>(depth), type, n_features,
                            capacity, report_out_dev, points_out, feature_out);
}

}  // extern "C"
