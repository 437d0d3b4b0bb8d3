// mld_row_growth.hip — the reference's second depth segmentation, region growing along lidar rows, for a batch of sequences
// (include/mld.h, "mld_row_growth"): HelperLidarRowSegmentation (SegmentPoints, calculateNeighborPoints) and the branch of
// DepthEstimator::CalculateDepth that do_use_depth_segmentation: 1 selects (DepthEstimator.cpp:512-558), which the
// reference ships behind a throw (:608).  The inputs are the arrays mld_projected_clouds_export_device writes (visible uv,
// n_visible, pixel map, _pointIndex, camera-frame cloud).  No frame slot is involved, nothing is allocated per call, nothing
// comes back to the host, no atomics, no floating-point accumulation.
//
// The cloud stage, once per cloud: the descriptor upload and
//   k_rg_pass    grid (sequence, chunk of 1024 visible points): point i opens a row iff i == 0 or x_i > x_{i-1} + 50
//                (HelperLidarRowSegmentation.cpp:26-43); one 64-bit mask of the breaks per 64 points, the breaks of the chunk,
//                and (first break, last break, widest gap between two breaks) of the chunk
//   k_rg_scan    one block per sequence: the prefix of the chunk counts, the chunks' (first, last, gap) folded into the
//                longest row, the 16-byte record, row_start[n_rows] = n_vis where nothing was truncated
//   k_rg_write   grid (sequence, chunk): the rank of a break is its row; row_start[row] = i for row <= row_capacity
// The feature stage: the descriptor upload and
//   k_row_growth grid (sequence, feature), ONE WAVEFRONT PER FEATURE:
//     G1  the narrow window's list (gather_window of ../batch/mld_depth_path.h), the count test
//     G2  the seed: CalculateNearestPoint's fold with its FLOAT accumulator (DepthEstimator.cpp:703-712), 64 entries per
//         step by repeated ballot - the first lane whose z beats m, then the lanes behind it
//     G3  the seed's row by binary search in row_start (uniform loads); the crossing search of getSingleNeighborRowPoint on
//         the rows above and below, 64 columns per step with the previous column from the neighbouring lane and a carry
//         between steps, both rows' loads in flight; getNeighborRowPoint's order, selectRowIndex
//     G4  getSelectionFromSeed twice on one list in LDS.  Unbounded (count -1): 64 points per step - index and cam gathered,
//         both distances per lane (`last` from the neighbouring lane), a ballot for the first failure; up the columns, then
//         down WITHOUT resetting `last` (HelperLidarRowSegmentation.cpp:205).  Bounded: the two-pointer merge, wave-uniform
//         and serial, at most 256 steps
//     G5  CalculateDepthSegmented on the grown list: max_spanning_triangle or the first three, list_minmax_z, finish_main
//         (../batch/mld_depth_path.h); the record is staged in LDS by lane 0 and leaves as one store of a dword per lane
//
// Per block of k_row_growth (one wavefront), from the compiler's resource report for gfx950
// (-Rpass-analysis=kernel-resource-usage):
//   LDS       dynamic, 28 E + 72 bytes with E = max(cells the wide window can cover, list entries) rounded up to even; list
//             entries: 1024 with count -1, else max(count, 2).  C0 (the wide window can cover 14 x 15 = 210 cells), count 4:
//             5 952 bytes; count -1: 28 744 bytes
//   VGPRs     103 (both instantiations), 106 SGPRs; SGPR spills go to VGPR lanes
//   scratch   0
//   wavefronts per CU   16 by registers (4 per SIMD); by LDS (160 KiB per CU) 5 with count -1, the register bound with a
//             bounded count
// The cloud stage: k_rg_pass 20 VGPRs and 144 bytes of LDS, k_rg_scan 28 and 3 088, k_rg_write 17 and none; scratch 0.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with it
// (descriptor ring, compaction scratch and object skeleton: ../batch/mld_batch_object.h; as_global, V3, the wavefront
// helpers, the pieces of the pass / scan / write compaction: ../batch/mld_batch_device.h; the window scan, the corners, the
// tail, the calibration, the refusals, the skeleton of a unit with one wavefront per feature: ../batch/mld_depth_path.h).  It
// is compiled without contraction like the rest of the library; the records are bit for bit what the CPU restatement
// computes (tests/test_row_growth_gpu.py pins that).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"
#include "../batch/mld_depth_path.h"
#include "../../../include/mld.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;
constexpr int kGroupsPerWave = 4;                // consecutive groups of 64 points a wavefront takes
constexpr int kChunk = kBlock * kGroupsPerWave;  // 1024 points = 16 groups per block
constexpr int kGroupsPerChunk = kChunk / kWave;
constexpr double kRowJump = 50.0;                // HelperLidarRowSegmentation.cpp:30
constexpr double kNoPoint = (double)INT_MIN;     // lastX (:26), lastPoint.x (:75)

static_assert(sizeof(mld_row_growth) == 72, "72 bytes per record (include/mld.h)");
static_assert(offsetof(mld_row_growth, corner_vis) == 44 && offsetof(mld_row_growth, depth) == 56 &&
                  offsetof(mld_row_growth, seed_z) == 64 && alignof(mld_row_growth) == 8,
              "field offsets of the record (include/mld.h)");
static_assert(sizeof(mld_row_growth_cloud) == 16 && sizeof(mld_row_growth_params) == 64, "include/mld.h");
static_assert(MLD_ROW_GROWTH_MAX_LIST == kMaxCells && MLD_ROW_GROWTH_MAX_COUNT == 256, "the lists and the LDS budget assume them");

// One sequence of a segment call.  Host-made, staged through a descriptor ring.
struct RgCloud {
    const double* uv;         // 2 x capacity: (u, v) of visible point r
    const int64_t* n_vis;     // the sequence's entry of n_visible (device memory)
    int32_t* row_start;       // row_capacity + 1
    mld_row_growth_cloud* rec;
    int32_t capacity;         // points uv holds
    int32_t pad_;
};
static_assert(sizeof(RgCloud) == 40, "40 bytes per sequence (include/mld.h)");

// One sequence of a collect call.
struct RgSeq {
    const void* u;         // uv, 2 x n_feat f64 (collect_device); u, n_feat f32 (collect_tracks_device)
    const float* v;        // tracks form only
    const int32_t* map;    // W * H: visible index or -1
    const int32_t* index;  // index_len: original index of a visible point
    const double* cam;     // 3 x n_points
    const double* vis_uv;  // 2 x index_len: (u, v) of a visible point
    const int32_t* row_start;
    const mld_row_growth_cloud* cloud;
    mld_row_growth* rec;
    int32_t* grown;        // list_capacity x n_feat, or null
    void* depth_io;        // n_feat f64 (f32 in the tracks form), or null
    int32_t* type_io;      // n_feat, or null
    int32_t n_feat;
    int32_t index_len;
    int32_t n_points;
    int32_t pad_;
};
static_assert(sizeof(RgSeq) == 112, "112 bytes per sequence (include/mld.h)");

// The visible points of a sequence the kernels may read: what was counted, and no more than the array holds.
__device__ __forceinline__ int visible_points(const RgCloud& q) {
    const long long n = *as_global(q.n_vis);
    return (int)(n < 0 ? 0 : (n > (long long)q.capacity ? (long long)q.capacity : n));
}

// ---- the cloud stage

// (first break, last break, widest gap between consecutive breaks) of a run of points; first == -1: no break.
struct Gaps {
    int first, last, widest;
};
__device__ __forceinline__ Gaps join(Gaps a, Gaps b) {
    if (a.first < 0) return b;
    if (b.first < 0) return a;
    return {a.first, b.last, max(max(a.widest, b.widest), b.first - a.last)};
}

// Grid (sequence, chunk of 1024 points).  gm: one 64-bit mask of the breaks per 64 points; cpre[c + 1]: the breaks of chunk
// c (k_rg_scan makes them a prefix); gaps[3 c ..]: first, last and widest of chunk c.
__global__ __launch_bounds__(kBlock) void k_rg_pass(const RgCloud* __restrict__ desc, unsigned long long* __restrict__ gm_all,
                                                   long long groups_per_seq, int* __restrict__ cpre_all, long long chunks_per_seq,
                                                   int* __restrict__ gaps_all) {
    __shared__ int wsum[kBlock / kWave];
    __shared__ unsigned long long masks[kGroupsPerChunk];
    const RgCloud q = desc[blockIdx.x];
    const int n = visible_points(q);
    if ((int)blockIdx.y * kChunk >= n) return;  // (uniform in the block)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = uniform((int)threadIdx.x >> 6);
    const int first = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave * kWave;  // the wavefront's first point
    const MLD_BATCH_GLOBAL double* uv = as_global(q.uv);
    unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    // the loads of the wavefront's groups first: a point and the one ahead of it
    double x[kGroupsPerWave], xp[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        x[k] = i < n ? uv[2 * (size_t)i] : 0.0;
        xp[k] = (i < n && i > 0) ? uv[2 * (size_t)(i - 1)] : kNoPoint;
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave, i = i0 + lane;
        const unsigned long long m = __ballot(i < n && (i == 0 || x[k] > xp[k] + kRowJump));
        if (lane == 0) {
            masks[wave * kGroupsPerWave + k] = m;
            if (i0 < n) *as_global(gm + (i0 >> 6)) = m;
        }
        cnt += (int)__popcll(m);
    }
    if (lane == 0) wsum[wave] = cnt;
    chunk_count(wsum, cpre_all, chunks_per_seq);  // (a barrier: the masks are in LDS)
    if (threadIdx.x == 0) {
        Gaps g = {-1, -1, 0};
        const int base = (int)blockIdx.y * kChunk;
#pragma unroll 1
        for (int k = 0; k < kGroupsPerChunk; k++) {
            unsigned long long m = masks[k];
            while (m != 0ull) {  // one step per break
                const int i = base + k * kWave + (int)__ffsll((long long)m) - 1;
                g = join(g, Gaps{i, i, 0});
                m &= m - 1ull;
            }
        }
        MLD_BATCH_GLOBAL int* out = as_global(gaps_all + ((size_t)blockIdx.x * (size_t)chunks_per_seq + blockIdx.y) * 3);
        out[0] = g.first, out[1] = g.last, out[2] = g.widest;
    }
}

// One block per sequence.  cpre becomes the rows ahead of every chunk; the record; row_start[n_rows] = n_vis.
__global__ __launch_bounds__(256) void k_rg_scan(const RgCloud* __restrict__ desc, int* cpre_all, long long chunks_per_seq,
                                                const int* __restrict__ gaps_all, int row_capacity) {
    __shared__ Gaps part[256];
    const RgCloud q = desc[blockIdx.x];
    const int n = visible_points(q);
    const int NC = (n + kChunk - 1) / kChunk;
    int* cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1);
    const int n_rows = scan_chunk_counts(cpre, NC);
    // the longest row: every thread folds a run of consecutive chunks, thread 0 the 256 runs in order
    const int tid = (int)threadIdx.x;
    const int per = (NC + 255) / 256;
    const int* gaps = gaps_all + (size_t)blockIdx.x * (size_t)chunks_per_seq * 3;
    Gaps g = {-1, -1, 0};
    for (int c = tid * per; c < min((tid + 1) * per, NC); c++) g = join(g, Gaps{gaps[3 * c], gaps[3 * c + 1], gaps[3 * c + 2]});
    part[tid] = g;
    __syncthreads();
    if (tid == 0) {
        Gaps all = {-1, -1, 0};
        for (int t = 0; t < 256; t++) all = join(all, part[t]);
        const int longest = all.first < 0 ? 0 : max(all.widest, n - all.last);  // (the last row ends with the cloud)
        MLD_BATCH_GLOBAL int32_t* rec = as_global(reinterpret_cast<int32_t*>(q.rec));
        rec[0] = n_rows;
        rec[1] = n;
        rec[2] = longest;
        rec[3] = n_rows > row_capacity ? MLD_ROW_GROWTH_FLAG_ROWS_TRUNCATED : 0;
        if (n_rows <= row_capacity) as_global(q.row_start)[n_rows] = n;
    }
}

// Grid (sequence, chunk of 1024 points): row_start[rank of the break] = the point, for the ranks up to row_capacity (the
// entry at row_capacity of a truncated sequence is the start of the first row that did not fit).
__global__ __launch_bounds__(kBlock) void k_rg_write(const RgCloud* __restrict__ desc, const unsigned long long* __restrict__ gm_all,
                                                    long long groups_per_seq, const int* __restrict__ cpre_all, long long chunks_per_seq,
                                                    int row_capacity) {
    const RgCloud q = desc[blockIdx.x];
    const int n = visible_points(q);
    const int b = (int)blockIdx.y;
    if (b * kChunk >= n) return;  // (uniform in the block)
    const int base = cpre_all[(size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) + b];  // rows ahead of the chunk
    if (base > row_capacity) return;  // nothing of this chunk is stored (uniform in the block)
    const unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = uniform((int)threadIdx.x >> 6);
    const int G = (n + kWave - 1) / kWave;
    const int g_mine = b * kGroupsPerChunk + lane;  // lanes 0..15: the masks of the block
    const unsigned long long mine = (lane < kGroupsPerChunk && g_mine < G) ? gm[g_mine] : 0ull;
    unsigned lo[kGroupsPerWave], hi[kGroupsPerWave];
    int first_rank[kGroupsPerWave];
    group_ranks<kGroupsPerChunk>(mine, base, lane, wave, lo, hi, first_rank);
    const int first = (b * kGroupsPerChunk + wave * kGroupsPerWave) * kWave;  // the wavefront's first point
    MLD_BATCH_GLOBAL int32_t* row_start = as_global(q.row_start);
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        const unsigned long long m = ((unsigned long long)hi[k] << 32) | lo[k];
        const int rank = first_rank[k] + lane_rank(lo[k], hi[k]);
        if (((m >> lane) & 1ull) && rank <= row_capacity) row_start[rank] = i;  // (a set bit is a point below n)
    }
}

// ---- the feature stage

// What the reference's calculateNeighborPoints takes besides the cloud, as the kernel takes it.
struct Growth {
    double thr;                  // depth_segmentation_max_treshold_gradient
    double s2s_start, s2s_grad;  // seedpoint to seedpoint
    double n2s_start, n2s_grad;  // neighbor to seedpoint
    double nb_start, nb_grad;    // neighbor
    int32_t count;
    int32_t row_capacity;
};

// HelperLidarRowSegmentation::getMaxDist (:302-313): the delta is taken from the START VALUE, not from the threshold
__device__ __forceinline__ double max_dist(double thr, double start, double grad, double z_seed) {
    if (z_seed <= thr) return start;
    const double delta = z_seed - start;
    return start + delta * grad;
}

// PointcloudData::CalcDistance (PointcloudData.h:42-44): pow(d, 2) is d * d, summed left to right
__device__ __forceinline__ double dist3(V3 a, V3 b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}
__device__ __forceinline__ double sqdist2(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}

// get3DPointFromCut of the visible point p (0 <= p < index_len): false where its index lies outside the cloud.
__device__ __forceinline__ bool point3(const RgSeq& q, int p, V3& out) {
    const int o = as_global(q.index)[p];
    if (o < 0 || o >= q.n_points) return false;
    const MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    out = {cam[3 * (size_t)o], cam[3 * (size_t)o + 1], cam[3 * (size_t)o + 2]};
    return true;
}

// A row of the segmentation: the visible points [start, end).  Values that leave [0, lim] or run backwards: an empty row
// and `bad`.
struct Row {
    int start, end;
};
__device__ __forceinline__ Row row_range(const RgSeq& q, int r, int lim, bool& bad) {
    const MLD_BATCH_GLOBAL int32_t* rs = as_global(q.row_start);
    const int s = uniform(rs[r]), e = uniform(rs[r + 1]);
    if (s < 0 || e > lim || s > e) {
        bad = true;
        return {0, 0};
    }
    return {s, e};
}

// G2: CalculateNearestPoint (DepthEstimator.cpp:703-712) over the first n list entries: `float m = +inf; for i: if (z_i <
// (double)m) { m = (float)z_i; idx = i; }`.  The position of the seed in the list, or -1.
__device__ __forceinline__ int seed_fold(int n, const PointList& L, int lane) {
    float m = __builtin_inff();
    int idx = -1;
    for (int base = 0; base < n; base += kWave) {  // (uniform)
        const int i = base + lane;
        const double z = i < n ? L.z[i] : __builtin_nan("");
        unsigned long long behind = ~0ull;  // the lanes the serial loop has not passed yet
        for (;;) {
            const unsigned long long beat = __ballot(z < (double)m) & behind;
            if (beat == 0ull) break;
            const int first = (int)__ffsll((long long)beat) - 1;
            m = (float)__shfl(z, first);
            idx = base + first;
            behind = first == kWave - 1 ? 0ull : (~0ull << (first + 1));
        }
    }
    return uniform(idx);
}

// G3: getSingleNeighborRowPoint (:68-107) on the rows a and b at once: the first column c with x_c < fx && x_{c-1} >= fx
// (x_{-1} = INT_MIN), then c or c - 1.  The visible index per row, -1 without a crossing.
__device__ __forceinline__ void crossings(const RgSeq& q, Row a, Row b, double fx, double fy, int lane, int& out_a, int& out_b) {
    const MLD_BATCH_GLOBAL double* uv = as_global(q.vis_uv);
    int ca = -1, cb = -1;
    bool open_a = a.start < a.end, open_b = b.start < b.end;
    double carry_a = kNoPoint, carry_b = kNoPoint;
    for (int off = 0; open_a || open_b; off += kWave) {  // (uniform)
        const int pa = a.start + off + lane, pb = b.start + off + lane;
        const bool in_a = open_a && pa < a.end, in_b = open_b && pb < b.end;
        const double xa = in_a ? uv[2 * (size_t)pa] : __builtin_nan("");
        const double xb = in_b ? uv[2 * (size_t)pb] : __builtin_nan("");
        if (open_a) {
            double prev = __shfl_up(xa, 1);
            if (lane == 0) prev = carry_a;
            const unsigned long long hit = __ballot(in_a && xa < fx && prev >= fx);
            if (hit != 0ull) {
                ca = a.start + off + (int)__ffsll((long long)hit) - 1;
                open_a = false;
            } else {
                carry_a = __shfl(xa, kWave - 1);
                open_a = a.start + off + kWave < a.end;
            }
        }
        if (open_b) {
            double prev = __shfl_up(xb, 1);
            if (lane == 0) prev = carry_b;
            const unsigned long long hit = __ballot(in_b && xb < fx && prev >= fx);
            if (hit != 0ull) {
                cb = b.start + off + (int)__ffsll((long long)hit) - 1;
                open_b = false;
            } else {
                carry_b = __shfl(xb, kWave - 1);
                open_b = b.start + off + kWave < b.end;
            }
        }
    }
    auto pick = [&](Row r, int c) {  // :97-106
        c = uniform(c);
        if (c < 0) return -1;
        if (c == r.start) return c;  // indexLast == -1
        const double cx = uv[2 * (size_t)c], cy = uv[2 * (size_t)c + 1];
        const double lx = uv[2 * (size_t)(c - 1)], ly = uv[2 * (size_t)(c - 1) + 1];
        // the second distance is between the two returns, not to the feature
        return sqdist2(cx, cy, fx, fy) < sqdist2(cx, cy, lx, ly) ? c : c - 1;
    };
    out_a = pick(a, ca);
    out_b = pick(b, cb);
}

struct GrowLists : PointList {
    int32_t* vis;  // visible index of list entry i
    int cap;       // entries the lists hold
};

// G4, count < 0 (:179-229): up the columns from the seed at p0 in row r, or down (kUp false), until the row ends, d(p, seed) >
// max_seed or d(p, last) > max_nb.  The accepted points go behind the n entries of the list (the first L.cap are kept,
// n counts them all); `last` is the caller's and stays what it is at the end.
template <bool kUp>
__device__ __forceinline__ void grow_unbounded(const RgSeq& q, const GrowLists& L, Row r, int p0, V3 seed, double max_nb, double max_seed,
                                               int lane, int& n, V3& last, bool& bad) {
    const int steps = kUp ? r.end - 1 - p0 : p0 - r.start;  // points on this side of the seed
    for (int off = 0; off < steps; off += kWave) {  // (uniform)
        const int k = off + lane;
        const int p = kUp ? p0 + 1 + k : p0 - 1 - k;
        const bool in = k < steps;
        V3 P = {0.0, 0.0, 0.0};
        const bool ok = in && point3(q, p, P);
        V3 prev = {__shfl_up(P.x, 1), __shfl_up(P.y, 1), __shfl_up(P.z, 1)};
        if (lane == 0) prev = last;
        const bool fail = !ok || dist3(P, seed) > max_seed || dist3(P, prev) > max_nb;
        const unsigned long long stop = __ballot(fail);
        const int taken = stop != 0ull ? (int)__ffsll((long long)stop) - 1 : kWave;
        if (lane < taken && n + lane < L.cap) {
            L.x[n + lane] = P.x;
            L.y[n + lane] = P.y;
            L.z[n + lane] = P.z;
            L.vis[n + lane] = p;
        }
        n += taken;
        if (taken > 0) last = {__shfl(P.x, taken - 1), __shfl(P.y, taken - 1), __shfl(P.z, taken - 1)};
        if (stop != 0ull) {
            if (__shfl((int)(in && !ok), taken)) bad = true;  // the point the walk ended at has an index outside the cloud
            break;
        }
    }
}

// G4, count >= 0 (:230-274): the two-pointer merge by distance to the seed, '<=' takes the upper side; it ends when EITHER
// side runs out, the taken point is farther than max_seed, or the list has reached `count` entries.  Wave-uniform.
__device__ __forceinline__ void grow_bounded(const RgSeq& q, const GrowLists& L, Row r, int p0, V3 seed, double max_seed, int count,
                                             int lane, int& n, bool& bad) {
    int pos = p0 + 1, neg = p0 - 1;
    for (;;) {
        if (pos >= r.end) break;
        if (neg < r.start) break;
        V3 Pp, Pn;
        if (!point3(q, pos, Pp) || !point3(q, neg, Pn)) {
            bad = true;
            break;
        }
        const double dp = dist3(Pp, seed), dn = dist3(Pn, seed);
        const bool up = dp <= dn;
        const V3 P = up ? Pp : Pn;
        const int p = up ? pos : neg;
        if (up) pos++; else neg--;
        if ((up ? dp : dn) > max_seed) break;
        if (lane == 0 && n < L.cap) {  // (n < max(count, 2) <= L.cap)
            L.x[n] = P.x;
            L.y[n] = P.y;
            L.z[n] = P.z;
            L.vis[n] = p;
        }
        n++;
        if (n >= count) break;
    }
}

template <bool kTracks>
__device__ __forceinline__ void grow_feature(const DepthCalib& c, const Growth& g, const RgSeq& q, const GrowLists& L, mld_row_growth* rec,
                                             const int f, const int lane, const int list_cap) {
    double u, v;
    read_feature<kTracks>(q.u, q.v, f, u, v);
    const MLD_BATCH_GLOBAL int32_t* cloud = as_global(reinterpret_cast<const int32_t*>(q.cloud));
    const int n_rows_all = uniform(cloud[0]), n_vis = uniform(cloud[1]);
    const int lim = min(max(n_vis, 0), q.index_len);  // visible points whose uv and index may be read
    int type = MLD_Unspecified, state = 0, grown_type = 0, flags = 0;
    int n_nb = 0, seed_vis = -1, second_vis = -1, seed_row = -1, second_row = -1, n_first = 0, n_grown = 0;
    int cv0 = -1, cv1 = -1, cv2 = -1;
    double depth = -1.0, seed_z = __builtin_nan("");
    bool bad = false;
    do {  // (every condition below is wave-uniform)
        if (n_rows_all > g.row_capacity) {
            flags |= MLD_ROW_GROWTH_FLAG_ROWS_TRUNCATED;
            break;
        }
        if (!(isfinite(u) && isfinite(v))) {
            flags |= MLD_ROW_GROWTH_FLAG_NONFINITE_FEATURE;
            type = MLD_RadiusSearchInsufficientPoints;
            break;
        }
        // ---- G1 (DepthEstimator.cpp:509-510)
        n_nb = gather_window(c, q, u, v, c.halfX1, c.halfY1, L, lane, bad, [&](int rank, int m, int) { L.vis[rank] = m; });
        __syncthreads();
        if ((unsigned)n_nb < c.countMin) {
            type = MLD_RadiusSearchInsufficientPoints;
            break;
        }
        // ---- G2 (:522-527)
        const int at = seed_fold(n_nb, L, lane);
        if (at < 0) {
            type = MLD_HistogramNoLocalMax;
            break;
        }
        const V3 seed = list_point(L, at);
        seed_vis = L.vis[at];
        seed_z = seed.z;
        __syncthreads();  // (the list is free from here on)
        if (seed.z > c.thrG_max) {  // whether or not treshold_depth_enabled is set
            type = MLD_TresholdDepthGlobalGreaterMax;
            break;
        }
        // ---- G3: the seed's row (getRowFromPoint), the largest r with row_start[r] <= seed_vis
        const int n_rows = n_rows_all;
        if (n_rows < 1 || seed_vis >= lim) {
            bad = true;
            break;
        }
        {
            const MLD_BATCH_GLOBAL int32_t* rs = as_global(q.row_start);
            int lo = 0, hi = n_rows;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (uniform(rs[mid]) <= seed_vis) lo = mid; else hi = mid;
            }
            seed_row = lo;
        }
        const Row row1 = row_range(q, seed_row, lim, bad);
        if (!(row1.start <= seed_vis && seed_vis < row1.end)) {
            bad = true;
            break;
        }
        // getNeighborRowPoint (:109-157)
        const double fx = u, fy = v;
        const Row top = seed_row >= 1 ? row_range(q, seed_row - 1, lim, bad) : Row{0, 0};
        const Row bottom = seed_row + 1 < n_rows ? row_range(q, seed_row + 1, lim, bad) : Row{0, 0};
        int i_top, i_bottom;
        crossings(q, top, bottom, fx, fy, lane, i_top, i_bottom);
        int cand0 = -1, cand1 = -1;
        if (i_top < 0 && i_bottom < 0) {
            state = -1;
            break;
        } else if (i_bottom < 0) {
            cand0 = i_top;
        } else if (i_top < 0) {
            cand0 = i_bottom;
        } else {
            const MLD_BATCH_GLOBAL double* uv = as_global(q.vis_uv);
            const double d_top = sqdist2(uv[2 * (size_t)i_top], uv[2 * (size_t)i_top + 1], fx, fy);
            const double d_bottom = sqdist2(uv[2 * (size_t)i_bottom], uv[2 * (size_t)i_bottom + 1], fx, fy);
            const bool top_first = d_top < d_bottom;  // a tie puts the bottom row first
            cand0 = top_first ? i_top : i_bottom;
            cand1 = top_first ? i_bottom : i_top;
        }
        // selectRowIndex (:277-300)
        const double max_s2s = max_dist(g.thr, g.s2s_start, g.s2s_grad, seed.z);
        V3 P2;
        if (point3(q, cand0, P2)) {
            if (dist3(seed, P2) <= max_s2s) second_vis = cand0;
        } else {
            bad = true;
        }
        if (second_vis < 0 && cand1 >= 0) {
            if (point3(q, cand1, P2)) {
                if (dist3(seed, P2) <= max_s2s) second_vis = cand1;
            } else {
                bad = true;
            }
        }
        if (second_vis < 0) {
            state = -2;
            break;
        }
        second_row = second_vis == i_top ? seed_row - 1 : seed_row + 1;
        const Row row2 = second_vis == i_top ? top : bottom;
        // ---- G4 (:354-374).  The call sites hand (maxDistNeighborToSeed, maxDistNeighbor) to the parameters named
        // (maxDistanceNeighbor, maxDistanceSeed): the roles are swapped, and stay so.
        const double max_nb = max_dist(g.thr, g.n2s_start, g.n2s_grad, seed.z);
        const double max_seed = max_dist(g.thr, g.nb_start, g.nb_grad, seed.z);
        int n = 0;
        if (g.count < 0) {
            V3 last = seed;
            grow_unbounded<true>(q, L, row1, seed_vis, seed, max_nb, max_seed, lane, n, last, bad);
            grow_unbounded<false>(q, L, row1, seed_vis, seed, max_nb, max_seed, lane, n, last, bad);
            n_first = n;
            last = P2;
            grow_unbounded<true>(q, L, row2, second_vis, P2, max_nb, max_seed, lane, n, last, bad);
            grow_unbounded<false>(q, L, row2, second_vis, P2, max_nb, max_seed, lane, n, last, bad);
        } else {
            grow_bounded(q, L, row1, seed_vis, seed, max_seed, g.count / 2, lane, n, bad);
            n_first = n;
            grow_bounded(q, L, row2, second_vis, P2, max_seed, g.count, lane, n, bad);
        }
        n_grown = uniform(n);
        state = n_grown == n_first ? -3 : 1;
        __syncthreads();
        if (q.grown) {
            MLD_BATCH_GLOBAL int32_t* row = as_global(q.grown) + (size_t)f * (size_t)list_cap;
            for (int i = lane; i < min(min(n_grown, L.cap), list_cap); i += kWave) row[i] = L.vis[i];
        }
        if (n_grown > L.cap) {  // (only unbounded growth gets there: L.cap is MLD_ROW_GROWTH_MAX_LIST then)
            flags |= MLD_ROW_GROWTH_FLAG_LIST_CAPPED;
            break;
        }
        if (state != 1) break;
        // ---- G5: CalculateDepthSegmented (:903-1036) on the grown list: no count test, no histogram
        int ci = 0, cj = 1, ck = 2;
        if (c.useTriMax) {
            if (!max_spanning_triangle(n_grown, L, lane, ci, cj, ck)) {
                grown_type = MLD_TriangleNotPlanarInsufficientPoints;
                break;
            }
        } else if (n_grown < 3) {
            grown_type = MLD_HistogramNoLocalMax;  // :920-921
            break;
        }
        cv0 = L.vis[ci], cv1 = L.vis[cj], cv2 = L.vis[ck];
        double mn, mx, d;
        list_minmax_z(n_grown, L, lane, mn, mx);
        grown_type = finish_main(c, u, v, list_point(L, ci), list_point(L, cj), list_point(L, ck), mn, mx, nullptr, d);
        if (grown_type == MLD_Success) {
            type = MLD_SuccessRegionGrowing;
            depth = d;
        }
    } while (false);
    if (bad) flags |= MLD_ROW_GROWTH_FLAG_BAD_INPUT;

    // ---- the record: staged by lane 0, stored as one dword per lane; the merge into the product's outputs
    __syncthreads();
    if (lane == 0) {
        rec->type = type;
        rec->state = state;
        rec->grown_type = grown_type;
        rec->flags = flags;
        rec->n_nb = n_nb;
        rec->seed_vis = seed_vis;
        rec->second_vis = second_vis;
        rec->seed_row = seed_row;
        rec->second_row = second_row;
        rec->n_first = n_first;
        rec->n_grown = n_grown;
        rec->corner_vis[0] = cv0;
        rec->corner_vis[1] = cv1;
        rec->corner_vis[2] = cv2;
        rec->depth = depth;
        rec->seed_z = seed_z;
        const bool decides = type == MLD_SuccessRegionGrowing || type == MLD_TresholdDepthGlobalGreaterMax || type == MLD_HistogramNoLocalMax;
        if (decides && q.type_io) as_global(q.type_io)[f] = type;
        if (decides && q.depth_io) {
            if (kTracks)
                as_global(static_cast<float*>(q.depth_io))[f] = (float)depth;
            else
                as_global(static_cast<double*>(q.depth_io))[f] = depth;
        }
    }
    store_record(rec, q.rec + f, lane);
}

// Entries of the lists in LDS: the cells of the widest window the calibration allows, or the longest grown list.
inline int list_entries(const DepthCalib& c, int count) {
    const int grown = count < 0 ? MLD_ROW_GROWTH_MAX_LIST : (count > 2 ? count : 2);
    const int e = c.cap > grown ? c.cap : grown;
    return (e + 1) & ~1;
}
inline size_t lds_bytes_for(int entries) { return (size_t)entries * 28 + sizeof(mld_row_growth); }

// Grid (sequence, feature); one wavefront per block.
template <bool kTracks>
__global__ __launch_bounds__(kWave) void k_row_growth(const RgSeq* __restrict__ desc, DepthCalib c, Growth g, int entries, int list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RgSeq q = desc[blockIdx.x];
    const int lane = (int)threadIdx.x;
    GrowLists L;
    L.x = reinterpret_cast<double*>(smem);
    L.y = L.x + entries;
    L.z = L.y + entries;
    mld_row_growth* rec = reinterpret_cast<mld_row_growth*>(L.z + entries);
    L.vis = reinterpret_cast<int32_t*>(rec + 1);
    L.cap = entries;
    for (int f = (int)blockIdx.y; f < q.n_feat; f += (int)gridDim.y)  // (uniform in the block)
        grow_feature<kTracks>(c, g, q, L, rec, f, lane, list_cap);
}

char g_error[512] = "";  // refusals without an object: mld_row_growth_last_error(NULL)

// What only this object refuses, first; then what mld_create refuses of a parameter set, a camera and a transform, with
// its texts - but for do_use_depth_segmentation, which is this object's subject.
int refuse_config(const mld_params& P_in, const mld_camera& cam, const double T[12], std::string& why) {
    mld_params P = P_in;
    P.do_use_depth_segmentation = 0;
    if (P.do_use_PCA) {
        why = "do_use_PCA: the eigen-solve is a tolerance path, the records promise equality";
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    if (P.set_all_depths_to_zero) {
        why = "set_all_depths_to_zero: every depth is 0 there, the depth calls answer that without a kernel";
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    int code = refuse_modes(P, why);
    if (code == MLD_OK) code = refuse_window_and_image(P, cam, why);
    if (code == MLD_OK) code = refuse_intrinsics(cam, why);
    if (code == MLD_OK) code = refuse_transform(T, why);
    if (code == MLD_OK) code = refuse_wide_window_cells(P, cam, why);
    return code;
}

}  // namespace

struct mld_row_growth_unit : mld_batch::Object {
    int n_seq = 0, row_capacity = 0;
    int64_t max_features = 0, max_points = 0;
    DepthCalib calib{};
    Growth growth{};
    int entries = 0;
    size_t lds_bytes = 0;
    CompactScratch scratch;    // break mask per 64 points; breaks ahead of every chunk (+ the total)
    DeviceBuffer<int> d_gaps;  // per chunk: first break, last break, widest gap
    mld_batch::DescRing<RgCloud> cloud_ring;
    mld_batch::DescRing<RgSeq> ring;
};

namespace {

// Both collect calls: u_tab = uv (v_tab null) or u, v.
template <bool kTracks>
int collect(mld_row_growth_unit* rg, const char* fn, const void* const* u_tab, const float* const* v_tab, const int64_t* n_features,
            const int32_t* const* map, const int32_t* const* index, const int64_t* index_len, const double* const* cam,
            const int64_t* n_points, const double* const* vis_uv, const int32_t* const* row_start,
            const mld_row_growth_cloud* cloud_dev, int list_capacity, mld_row_growth* const* record_out, int32_t* const* grown_out,
            void* const* depth_io, int32_t* const* type_io) {
    if (!rg) return no_object(g_error, fn, "rg");
    auto refuse = [&](int code, const char* text) { return fail(rg, code, (std::string(fn) + ": " + text).c_str()); };
    auto bad_arg = [&](const char* text) { return refuse(MLD_ERR_INVALID_ARG, text); };
    const FeatureTables t = {u_tab, v_tab, n_features, map, index, index_len, cam, n_points};
    const char* bad;
    if ((bad = feature_table_fault<kTracks>(t))) return bad_arg(bad);
    if (!vis_uv) return bad_arg("null table vis_uv");
    if (!row_start) return bad_arg("null table row_start");
    if (!cloud_dev) return bad_arg("null cloud_dev");
    if (misaligned(cloud_dev, 3u)) return bad_arg("cloud_dev must be 4-byte aligned");
    if (!record_out) return bad_arg("null table record_out");
    if (list_capacity < 0 || list_capacity > MLD_ROW_GROWTH_MAX_LIST) return bad_arg("list_capacity must be in 0 .. 1024");
    const int S = rg->n_seq;
    const unsigned depth_mask = kTracks ? 3u : 7u;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if ((bad = feature_sign_fault(t, s))) return bad_arg(bad);
        if ((bad = feature_capacity_fault(t, s, rg->max_features))) return refuse(MLD_ERR_CAPACITY, bad);
        const int64_t n = n_features[s];
        if (n == 0) continue;  // (needs no arrays)
        if ((bad = feature_array_fault<kTracks>(t, s))) return bad_arg(bad);
        if (index_len[s] > 0 && !vis_uv[s]) return bad_arg("null array vis_uv of a sequence with features and index_len > 0");
        if (!row_start[s]) return bad_arg("null array row_start of a sequence with features");
        if (!record_out[s]) return bad_arg("null array record_out of a sequence with features");
        if ((bad = feature_alignment_fault<kTracks>(t, s))) return bad_arg(bad);
        if (misaligned(vis_uv[s], 7u)) return bad_arg("vis_uv must be 8-byte aligned");
        if (misaligned(row_start[s], 3u)) return bad_arg("row_start must be 4-byte aligned");
        if (misaligned(record_out[s], 7u)) return bad_arg("record_out must be 8-byte aligned");
        if (list_capacity > 0 && grown_out && misaligned(grown_out[s], 3u)) return bad_arg("grown_out must be 4-byte aligned");
        if (depth_io && misaligned(depth_io[s], depth_mask)) return bad_arg(kTracks ? "depth_io must be 4-byte aligned" : "depth_io must be 8-byte aligned");
        if (type_io && misaligned(type_io[s], 3u)) return bad_arg("type_io must be 4-byte aligned");
        if (n > longest) longest = n;
    }
    for (int s = 0; s < S; s++) {
        RgSeq& q = rg->ring.stage[(size_t)s];
        q = RgSeq{};
        const int64_t n = n_features[s];
        if (n == 0) continue;
        q.u = u_tab[s];
        q.v = kTracks ? v_tab[s] : nullptr;
        q.map = map[s];
        q.index = index[s];
        q.cam = cam[s];
        q.vis_uv = vis_uv[s];
        q.row_start = row_start[s];
        q.cloud = cloud_dev + s;
        q.rec = record_out[s];
        q.grown = (list_capacity > 0 && grown_out) ? grown_out[s] : nullptr;
        q.depth_io = depth_io ? depth_io[s] : nullptr;
        q.type_io = type_io ? type_io[s] : nullptr;
        q.n_feat = (int32_t)n;
        q.index_len = (int32_t)index_len[s];
        q.n_points = (int32_t)n_points[s];
    }
    dim3 grid;
    if (!feature_grid(S, longest, grid)) return MLD_OK;
    MLD_HIP(rg, hipSetDevice(rg->device));
    const int rc = rg->ring.upload(rg);
    if (rc) return rc;
    hipLaunchKernelGGL(k_row_growth<kTracks>, grid, dim3(kWave), rg->lds_bytes, rg->stream, rg->ring.d_desc.get(), rg->calib, rg->growth,
                       rg->entries, list_capacity);
    MLD_HIP(rg, hipGetLastError());
    return MLD_OK;
}

}  // namespace

extern "C" {

void mld_row_growth_params_default(mld_row_growth_params* g) {  // DepthEstimatorParameters.h:52-60
    if (!g) return;
    *g = mld_row_growth_params{};
    g->depth_segmentation_max_treshold_gradient = 0.0;
    g->depth_segmentation_max_neighbor_distance = 0.3;
    g->depth_segmentation_max_neighbor_distance_gradient = 0.0;
    g->depth_segmentation_max_neighbor_to_seedpoint_distance = 0.5;
    g->depth_segmentation_max_neighbor_to_seedpoint_distance_gradient = 0.0;
    g->depth_segmentation_max_seedpoint_to_seedpoint_distance = 0.5;
    g->depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient = 0.0;
    g->depth_segmentation_max_pointcount = 5;
}

void mld_row_growth_params_yaml(mld_row_growth_params* g) {  // parameters.yaml:77-91
    if (!g) return;
    *g = mld_row_growth_params{};
    g->depth_segmentation_max_treshold_gradient = 10.0;
    g->depth_segmentation_max_neighbor_distance = 0.2;
    g->depth_segmentation_max_neighbor_distance_gradient = 0.02;
    g->depth_segmentation_max_neighbor_to_seedpoint_distance = 0.5;
    g->depth_segmentation_max_neighbor_to_seedpoint_distance_gradient = 0.05;
    g->depth_segmentation_max_seedpoint_to_seedpoint_distance = 0.5;
    g->depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient = 0.05;
    g->depth_segmentation_max_pointcount = 4;
}

mld_row_growth_unit* mld_row_growth_create(mld_ctx* ctx, int n_seq, int64_t max_features, int64_t max_points, int row_capacity,
                                           const mld_params* params, const mld_row_growth_params* growth, const mld_camera* camera,
                                           const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_row_growth_create: n_seq must be in 1 .. 65536";
        if (max_features < 1 || max_features > kMaxFeatures) return "mld_row_growth_create: max_features must be in 1 .. 16777216";
        if (max_points < 1 || max_points > kMaxPoints) return "mld_row_growth_create: max_points must be in 1 .. 8388607";
        if (row_capacity < 1 || row_capacity > MLD_ROW_GROWTH_MAX_ROWS) return "mld_row_growth_create: row_capacity must be in 1 .. 65536";
        if (!ctx) return "mld_row_growth_create: null context";
        if (!params) return "mld_row_growth_create: null params";
        if (!growth) return "mld_row_growth_create: null growth";
        if (!camera) return "mld_row_growth_create: null camera";
        if (!T_cam_lidar) return "mld_row_growth_create: null T_cam_lidar";
        if (growth->depth_segmentation_max_pointcount < -1 || growth->depth_segmentation_max_pointcount > MLD_ROW_GROWTH_MAX_COUNT)
            return "mld_row_growth_create: depth_segmentation_max_pointcount must be -1 or in 0 .. 256";
        return nullptr;
    };
    const char* bad = refusal();
    std::string why;
    // (what is refused with a status of its own; still nothing of the context is used)
    const int code = bad ? MLD_OK : refuse_config(*params, *camera, T_cam_lidar, why);
    auto init = [&](mld_row_growth_unit* rg) {
        rg->n_seq = n_seq;
        rg->max_features = max_features;
        rg->max_points = max_points;
        rg->row_capacity = row_capacity;
        mld_params P = *params;
        P.do_use_depth_segmentation = 0;
        build_calib(rg->calib, P, *camera, T_cam_lidar);
        Growth& g = rg->growth;
        g.thr = growth->depth_segmentation_max_treshold_gradient;
        g.s2s_start = growth->depth_segmentation_max_seedpoint_to_seedpoint_distance;
        g.s2s_grad = growth->depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient;
        g.n2s_start = growth->depth_segmentation_max_neighbor_to_seedpoint_distance;
        g.n2s_grad = growth->depth_segmentation_max_neighbor_to_seedpoint_distance_gradient;
        g.nb_start = growth->depth_segmentation_max_neighbor_distance;
        g.nb_grad = growth->depth_segmentation_max_neighbor_distance_gradient;
        g.count = growth->depth_segmentation_max_pointcount;
        g.row_capacity = row_capacity;
        rg->entries = list_entries(rg->calib, g.count);
        rg->lds_bytes = lds_bytes_for(rg->entries);
        int rc;
        if ((rc = rg->cloud_ring.allocate(rg, n_seq))) return rc;
        if ((rc = rg->ring.allocate(rg, n_seq))) return rc;
        if ((rc = rg->scratch.allocate(rg, n_seq, max_points, kChunk, 1))) return rc;
        return rg->d_gaps.allocate(rg, (size_t)n_seq * (size_t)rg->scratch.chunks_per_seq * 3);
    };
    return mld_batch::create_object<mld_row_growth_unit>(g_error, "mld_row_growth_create", bad, ctx, status_out, init, code, why.c_str());
}

void mld_row_growth_destroy(mld_row_growth_unit* rg) { mld_batch::destroy_object(rg); }

const char* mld_row_growth_last_error(const mld_row_growth_unit* rg) { return rg ? rg->err.c_str() : g_error; }

int mld_row_growth_segment_device(mld_row_growth_unit* rg, const double* const* uv, const int64_t* capacity,
                                  const int64_t* n_visible_dev, int32_t* const* row_start_out, mld_row_growth_cloud* cloud_out_dev) {
    const char* fn = "mld_row_growth_segment_device";
    if (!rg) return no_object(g_error, fn, "rg");
    auto refuse = [&](int code, const char* text) { return fail(rg, code, (std::string(fn) + ": " + text).c_str()); };
    auto bad_arg = [&](const char* text) { return refuse(MLD_ERR_INVALID_ARG, text); };
    if (!uv) return bad_arg("null table uv");
    if (!capacity) return bad_arg("null table capacity");
    if (!n_visible_dev) return bad_arg("null n_visible_dev");
    if (misaligned(n_visible_dev, 7u)) return bad_arg("n_visible_dev must be 8-byte aligned");
    if (!row_start_out) return bad_arg("null table row_start_out");
    if (!cloud_out_dev) return bad_arg("null cloud_out_dev");
    if (misaligned(cloud_out_dev, 3u)) return bad_arg("cloud_out_dev must be 4-byte aligned");
    const int S = rg->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if (capacity[s] < 0) return bad_arg("negative capacity");
        if (capacity[s] > rg->max_points) return refuse(MLD_ERR_CAPACITY, "capacity exceeds the max_points of the object");
        if (capacity[s] > 0 && !uv[s]) return bad_arg("null array uv of a sequence with capacity");
        if (misaligned(uv[s], 7u)) return bad_arg("uv must be 8-byte aligned");
        if (!row_start_out[s]) return bad_arg("null array row_start_out");
        if (misaligned(row_start_out[s], 3u)) return bad_arg("row_start_out must be 4-byte aligned");
        if (capacity[s] > longest) longest = capacity[s];
    }
    for (int s = 0; s < S; s++) {
        RgCloud& q = rg->cloud_ring.stage[(size_t)s];
        q = RgCloud{};
        q.uv = uv[s];
        q.n_vis = n_visible_dev + s;
        q.row_start = row_start_out[s];
        q.rec = cloud_out_dev + s;
        q.capacity = (int32_t)capacity[s];
    }
    MLD_HIP(rg, hipSetDevice(rg->device));
    const int rc = rg->cloud_ring.upload(rg);
    if (rc) return rc;
    const CompactScratch& cs = rg->scratch;
    const RgCloud* desc = rg->cloud_ring.d_desc.get();
    const unsigned chunks = (unsigned)((longest + kChunk - 1) / kChunk);
    if (chunks > 0)
        hipLaunchKernelGGL(k_rg_pass, dim3((unsigned)S, chunks), dim3(kBlock), 0, rg->stream, desc, cs.d_gm.get(), cs.groups_per_seq,
                           cs.d_cpre.get(), cs.chunks_per_seq, rg->d_gaps.get());
    hipLaunchKernelGGL(k_rg_scan, dim3((unsigned)S), dim3(256), 0, rg->stream, desc, cs.d_cpre.get(), cs.chunks_per_seq,
                       rg->d_gaps.get(), rg->row_capacity);
    if (chunks > 0)
        hipLaunchKernelGGL(k_rg_write, dim3((unsigned)S, chunks), dim3(kBlock), 0, rg->stream, desc, cs.d_gm.get(), cs.groups_per_seq,
                           cs.d_cpre.get(), cs.chunks_per_seq, rg->row_capacity);
    MLD_HIP(rg, hipGetLastError());
    return MLD_OK;
}

int mld_row_growth_collect_device(mld_row_growth_unit* rg, const double* const* uv, const int64_t* n_features,
                                  const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                  const double* const* cam, const int64_t* n_points, const double* const* vis_uv,
                                  const int32_t* const* row_start, const mld_row_growth_cloud* cloud_dev, int list_capacity,
                                  mld_row_growth* const* record_out, int32_t* const* grown_out, double* const* depth_io,
                                  int32_t* const* type_io) {
    return collect<false>(rg, "mld_row_growth_collect_device", reinterpret_cast<const void* const*>(uv), nullptr, n_features, map, index,
                          index_len, cam, n_points, vis_uv, row_start, cloud_dev, list_capacity, record_out, grown_out,
                          reinterpret_cast<void* const*>(depth_io), type_io);
}

int mld_row_growth_collect_tracks_device(mld_row_growth_unit* rg, const float* const* u, const float* const* v,
                                         const int64_t* n_features, const int32_t* const* map, const int32_t* const* index,
                                         const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                         const double* const* vis_uv, const int32_t* const* row_start,
                                         const mld_row_growth_cloud* cloud_dev, int list_capacity, mld_row_growth* const* record_out,
                                         int32_t* const* grown_out, float* const* depth_io, int32_t* const* type_io) {
    return collect<true>(rg, "mld_row_growth_collect_tracks_device", reinterpret_cast<const void* const*>(u), v, n_features, map, index,
                         index_len, cam, n_points, vis_uv, row_start, cloud_dev, list_capacity, record_out, grown_out,
                         reinterpret_cast<void* const*>(depth_io), type_io);
}

}  // extern "C"
