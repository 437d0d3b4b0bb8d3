// mld_batch_device.h — the device side the batch objects have in common (mld_projected_clouds, mld_depth_reports,
// mld_plane_inliers, mld_ransac_planes, mld_semantic_planes: all of it; mld_feature_traces and the units of the coverage
// maps, the depth images and the region depths: as_global, V3, the constants and the wavefront helpers, the first three
// through mld_depth_path.h, which restates the per-feature depth path on top of this header):
// __device__ functions, types and constants only - no kernel, no state, no host code, and nothing of the depth path.
//   as_global, load_xyz, V3 / to_camera, smallest_eigvec      what the kernels of several units read and compute alike
//   prefix_count, uniform, wave_sum, wave_max, reduce_best    ballots and butterflies over one wavefront
//   scan_inclusive, chunk_count, scan_chunk_counts,           the pass / scan / write stream compaction: every kernel
//   group_ranks, lane_rank                                    keeps its own name, signature, grid and epilogue
// The host side of the compaction (the scratch arrays and their sizes) is mld_batch::CompactScratch in mld_batch_object.h.
// Every unit is compiled without contraction: the floating-point expressions below keep their operation order.  The
// scans take and return plain values and no helper takes a __restrict__ pointer: other forms changed the kernels'
// instruction counts (profiles/batch_device_header.md).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mld_batch {

constexpr int kWave = 64;
constexpr int64_t kMaxPoints = 8388607;    // points of a cloud
constexpr int64_t kMaxFeatures = 16777216;  // features of a sequence

// The arrays of a descriptor are GPU memory: said to the compiler, their accesses are global_* instead of flat_*.
#define MLD_BATCH_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ MLD_BATCH_GLOBAL T* as_global(T* p) {
    return (MLD_BATCH_GLOBAL T*)p;
}

// A cloud record's first 16 bytes as ONE load, with the 4-byte alignment the C-ABI asks for (gfx950 takes multi-dword
// global loads at any dword address).  Stride 32 reads the first half of its record the same way.  Index: int (never
// negative) or uint32_t.
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float4v float4u __attribute__((aligned(4)));

template <int kStride, typename Index>
__device__ __forceinline__ void load_xyz(const unsigned char* __restrict__ cloud, Index i, float& x, float& y, float& z) {
    const float4v r = *(const MLD_BATCH_GLOBAL float4u*)(cloud + (size_t)i * (size_t)kStride);
    x = r.x, y = r.y, z = r.z;
}

// ---- the wavefront: every lane must be at a call (cross-lane reads)
// Set bits of the ballot m below this lane's.
__device__ __forceinline__ int prefix_count(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// A value every lane holds alike, said to the compiler: it lives in a scalar register from here on.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Sum and maximum by the xor butterfly: at every step a lane and its partner combine the same two values, so every lane
// ends with the same bits.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// (value descending, id ascending) over the wavefront; every lane ends with the winner.  No lane holds a NaN: a
// candidate only ever replaces a lane's value by comparing greater.
__device__ __forceinline__ void reduce_best(double& v, int& id) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d);
        const int oi = __shfl_xor(id, d);
        if (ov > v || (ov == v && oi < id)) {
            v = ov;
            id = oi;
        }
    }
}

struct V3 {
    double x, y, z;
};

// Raw float point -> camera frame (DepthEstimator.cpp:169,173); T: lidar -> camera, row-major 3x4
__device__ __forceinline__ V3 to_camera(const double (&T)[12], double x, double y, double z) {
    V3 r;
    r.x = T[3] + ((T[0] * x + T[1] * y) + T[2] * z);
    r.y = T[7] + ((T[4] * x + T[5] * y) + T[6] * z);
    r.z = T[11] + ((T[8] * x + T[9] * y) + T[10] * z);
    return r;
}

// Symmetric 3x3 Jacobi (double), smallest eigenvector; s = xx,xy,xz,yy,yz,zz.  The one copy of the two plane units; the
// depth path keeps its own (rs_smallest_eigvec in mld_ransac.hip), which this header does not reach into.
__device__ inline void smallest_eigvec(const double s[6], double n0[3]) {
    double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (!(off > 1e-300) || off <= 1e-32 * diag) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double apq = a[p][q];
                if (apq == 0.0) continue;
                double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; k++) {
                    double akp = a[k][p], akq = a[k][q];
                    a[k][p] = cs * akp - sn * akq;
                    a[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 3; k++) {
                    double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = cs * apk - sn * aqk;
                    a[q][k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < 3; k++) {
                    double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
    // index of the smallest diagonal entry, ties resolved like a stable ascending sort of (d0,d1,d2)
    int i0 = 0;
    double d0 = a[0][0];
    if (a[1][1] < d0) {
        d0 = a[1][1];
        i0 = 1;
    }
    if (a[2][2] < d0) i0 = 2;
    n0[0] = v[0][i0];
    n0[1] = v[1][i0];
    n0[2] = v[2][i0];
}

// ---- stream compaction in three kernels (pass, scan, write) over chunks of kBlock * kGroupsPerWave items: the pass
// leaves one 64-bit mask per group of 64 items and the count of every chunk, the scan makes the counts of a sequence a
// prefix, the write ranks the set bits.  cpre of a sequence: chunks_per_seq + 1 counts.  (mld_plane_inliers counts two
// things side by side and keeps its own pass tail and scan loop around the two-value scan_inclusive.)

// Inclusive prefix of v over the first kWidth lanes of a wavefront.  Every lane must be here.
template <int kWidth>
__device__ __forceinline__ int scan_inclusive(int v, int lane) {
#pragma unroll
    for (int d = 1; d < kWidth; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// The same for two values side by side (the cross-lane reads of a step in flight together).
struct IntPair {
    int a, b;
};
template <int kWidth>
__device__ __forceinline__ IntPair scan_inclusive(int a, int b, int lane) {
#pragma unroll
    for (int d = 1; d < kWidth; d <<= 1) {
        const int t = __shfl_up(a, d), u = __shfl_up(b, d);
        if (lane >= d) a += t, b += u;
    }
    return {a, b};
}

// The tail of a pass kernel, grid (sequence, chunk), once lane 0 of every wavefront has put its count into wsum: thread 0
// sums them into cpre[chunk + 1].  Every thread of the block must be here (a barrier).
template <int kWaves>
__device__ __forceinline__ void chunk_count(const int (&wsum)[kWaves], int* cpre_all, long long chunks_per_seq) {
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) t += wsum[w];
        *as_global(cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) + blockIdx.y + 1) = t;
    }
}

// The core of a scan kernel, one block of 256 threads per sequence: exclusive prefix over the NC chunk counts, in place
// (cpre[c] = items ahead of chunk c).  The loop carries the sum over any number of chunks; returns the total.
__device__ __forceinline__ int scan_chunk_counts(int* cpre, int NC) {
    __shared__ int wsum[256 / kWave];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    if (tid == 0) cpre[0] = 0;
    int carry = 0;
    for (int c0 = 0; c0 < NC; c0 += 256) {  // (uniform)
        const int c = c0 + tid;
        const int incl = scan_inclusive<kWave>(c < NC ? cpre[c + 1] : 0, lane);
        if (lane == kWave - 1) wsum[w] = incl;
        __syncthreads();
        int off = carry, total = 0;
#pragma unroll
        for (int k = 0; k < 256 / kWave; k++) {
            off += k < w ? wsum[k] : 0;
            total += wsum[k];
        }
        if (c < NC) cpre[c + 1] = off + incl;
        carry += total;
        __syncthreads();
    }
    return carry;
}

// The prologue of a write kernel from the masks on: `mine` is the 64-bit mask of group `lane` of the block (lanes at and
// beyond kGroupsPerChunk: 0), base the items ahead of the block.  For each of the wavefront's groups k: the halves of its
// mask and the rank of its first set bit.  Every lane must be here (cross-lane reads).
template <int kGroupsPerChunk, int kGroupsPerWave>
__device__ __forceinline__ void group_ranks(unsigned long long mine, int base, int lane, int wave, unsigned (&lo)[kGroupsPerWave],
                                            unsigned (&hi)[kGroupsPerWave], int (&first_rank)[kGroupsPerWave]) {
    const int pop = (int)__popcll(mine);
    const int ahead = scan_inclusive<kGroupsPerChunk>(pop, lane) - pop;  // set bits of the block ahead of this lane's group
    const unsigned mine_lo = (unsigned)mine, mine_hi = (unsigned)(mine >> 32);
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int gl = wave * kGroupsPerWave + k;  // the group within the block
        lo[k] = (unsigned)__shfl((int)mine_lo, gl);
        hi[k] = (unsigned)__shfl((int)mine_hi, gl);
        first_rank[k] = base + __shfl(ahead, gl);
    }
}

// Set bits of the mask (lo, hi) below this lane's: with first_rank, the rank of the lane's item.
__device__ __forceinline__ int lane_rank(unsigned lo, unsigned hi) {
    return (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
}

}  // namespace mld_batch
