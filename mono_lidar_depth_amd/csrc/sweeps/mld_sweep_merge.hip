// mld_sweep_merge.hip — the last few lidar sweeps of a batch of sequences carried into the current lidar frame and
// concatenated, current sweep first (include/mld.h, "mld_sweep_merge"): per sequence every record of every sweep is
// transformed by its sweep's 3x4 matrix (f64 from the float coordinates, rounded to float once), dropped when the result
// is not finite or lies outside [min_range, max_range], and the rest written back to back as packed 16-byte records
// {x', y', z', intensity bits} in the order (sweep, index within the sweep).  The pixel map keeps the FIRST return of a
// cell (NeighborFinderPixel.cpp:38-55), so with the current sweep in front the older sweeps only fill cells it left empty.
// No frame slot is involved, clouds are read where they lie, nothing is allocated per call, nothing comes back to the
// host, no atomics.
//
// The items of a sequence are the concatenation of its sweeps.  Four launches, ordered by kernel boundaries alone:
//   upload      the descriptors, one per (sequence, sweep) (mld_batch::DescRing)
//   k_sm_pass   grid (sequence, 1024 items): the record's first 16 bytes as one load, the transform, the two tests; the
//               ballot of the kept items as one 64-bit word per 64 items and, side by side, the chunk's two drop counts
//   k_sm_scan   one block per sequence: exclusive prefixes of both counts, in place (the kept items ahead of chunk c are
//               1024 c minus both); the kept items of every sweep from those prefixes and the masks at the sweep borders
//   k_sm_write  grid as the pass plus one block: rank of a kept item = chunk base + popcounts of the chunk's earlier
//               words + prefix within its word.  Only the kept lanes below the capacity load their record again and
//               transform it again - deterministic f64, so they get what the pass got - and store the whole 16-byte
//               record, the sweep and the index within the sweep.  The last block of a sequence writes its record.
// A sweep's matrix is uniform over a wavefront: the kernels walk the sweeps that a group of 64 items touches in a loop
// that is uniform in the wavefront (one round wherever a group lies inside one sweep), and read the round's twelve
// entries, start and array through a uniform address - scalar loads into scalar registers, not one load per lane.  A
// lane takes the round whose sweep holds its item.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring, object skeleton and compaction scratch: ../batch/mld_batch_object.h; the compaction's device
// pieces: ../batch/mld_batch_device.h).  It is compiled without contraction like the rest of the library: the
// expressions below keep their operation order, which tests/sweep_merge_restatement.py restates in NumPy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;
constexpr int kGroupsPerWave = 4;                // consecutive groups of 64 items a wavefront takes
constexpr int kChunk = kBlock * kGroupsPerWave;  // 1024 items = 16 groups per block
constexpr int kGroupsPerChunk = kChunk / kWave;
constexpr int kMaxSweeps = MLD_SWEEP_MAX_SWEEPS;
constexpr int kRecordWords = (int)(sizeof(mld_sweep_merge_record) / 8);

static_assert(sizeof(mld_sweep_merge_record) == 112 && sizeof(mld_sweep_merge_record) % 8 == 0, "14 int64 (include/mld.h)");
static_assert(kMaxSweeps == 16, "kept[] of the record");

// One sweep of one sequence of one call, at [s * max_sweeps + j].  Host-made, staged through the descriptor ring
// (mld_batch::DescRing).  The fields of the sequence ride on its sweep 0.
struct SmSweep {
    const unsigned char* cloud;
    int32_t start, end;  // the sweep's items within the sequence: [start, end)
    int32_t identity;    // no matrix: the coordinates bit for bit
    int32_t n_sweeps;    // (sweep 0)
    double T[12];        // sweep -> current lidar frame, row-major 3x4
    unsigned char* merged;  // (sweep 0) 16 x capacity bytes, null: capacity 0
    uint8_t* sweep_out;     // (sweep 0) capacity, or null
    int32_t* orig_out;      // (sweep 0) capacity, or null
    int32_t n_items;        // (sweep 0) = end of the last sweep
    int32_t capacity;       // (sweep 0) min(capacity[s], n_items): a rank is below n_items
};
static_assert(sizeof(SmSweep) == 152, "152 bytes per sweep (DESIGN.md)");

struct SmGate {
    float lo2, hi2;  // min_range^2, max_range^2, made on the host in f32
};

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
typedef uint4v uint4u __attribute__((aligned(4)));

// The record of item i (start <= i < end of sweep d): its first 16 bytes as ONE load, 4-byte aligned as the C-ABI asks.
template <int kStride>
__device__ __forceinline__ uint4v load_record(const SmSweep& d, int i) {
    return *(const MLD_BATCH_GLOBAL uint4u*)(d.cloud + (size_t)(i - d.start) * (size_t)kStride);
}

// Where mld_pack_points_host takes the intensity: the fourth float of a 16-byte record, the fifth of a 32-byte one.
template <int kStride>
__device__ __forceinline__ unsigned load_intensity(const SmSweep& d, int i, unsigned w16) {
    if (kStride == 16) return w16;
    return *(const MLD_BATCH_GLOBAL unsigned*)(d.cloud + (size_t)(i - d.start) * (size_t)kStride + 16);
}

// x' = (float)(T[3] + (T[0] x + (T[1] y + T[2] z))), likewise y', z' (include/mld.h); no matrix: the bits as they are.
__device__ __forceinline__ void transform(const SmSweep& d, float& x, float& y, float& z) {
    if (d.identity) return;  // (uniform in the wavefront)
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    x = (float)(d.T[3] + (d.T[0] * xd + (d.T[1] * yd + d.T[2] * zd)));
    y = (float)(d.T[7] + (d.T[4] * xd + (d.T[5] * yd + d.T[6] * zd)));
    z = (float)(d.T[11] + (d.T[8] * xd + (d.T[9] * yd + d.T[10] * zd)));
}

// 0 kept, 1 not finite, 2 out of range (a record that is both counts as not finite).
__device__ __forceinline__ int verdict(SmGate g, float x, float y, float z) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return 1;
    const float r2 = x * x + (y * y + z * z);
    return (g.lo2 <= r2 && r2 <= g.hi2) ? 0 : 2;
}

// The sweeps of a group of 64 items [i0, i0 + 64) of a sequence of n items, i0 < n: `j` (uniform, carried from group to
// group of a wavefront, never backwards) is moved to the sweep that holds i0; the rounds then run j, j + 1, .. up to the
// sweep that holds the group's last item.  SM_ROUNDS(t) { body } runs body with t uniform; a lane whose item i lies in
// [sw[t].start, sw[t].end) takes that round.  Empty sweeps are rounds nobody takes.
#define SM_SEEK(sw, j, i0) \
    while (sw[j].end <= (i0)) j++
#define SM_ROUNDS(sw, j, t, last) for (int t = j, more_ = 1; more_; more_ = sw[t].end <= (last), t++)

// Grid (sequence, chunk of 1024 items).  gm: one 64-bit mask of the kept items per 64 items; cpre[2 (c + 1)],
// cpre[2 (c + 1) + 1]: the items of chunk c that are not finite and those out of range (k_sm_scan makes them prefixes).
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_sm_pass(const SmSweep* __restrict__ desc, int max_sweeps, SmGate gate,
                                                   unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                   int* __restrict__ cpre_all, long long chunks_per_seq) {
    __shared__ int wsum[2][kBlock / kWave];
    const SmSweep* __restrict__ sw = desc + (size_t)blockIdx.x * (size_t)max_sweeps;
    const int n = sw[0].n_items;
    if ((int)blockIdx.y * kChunk >= n) return;  // (uniform in the block; n < 2^23: no overflow)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = uniform((int)threadIdx.x >> 6);
    const int first = ((int)blockIdx.y * (kBlock / kWave) + wave) * kGroupsPerWave * kWave;  // the wavefront's first item
    unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    int cnt_nf = 0, cnt_or = 0;
    if (first < n) {  // (uniform in the wavefront)
        int j = 0;
        SM_SEEK(sw, j, first);
        // the loads of the wavefront's groups first: up to four records per lane in flight
        uint4v rec[kGroupsPerWave];
        {
            int jl = j;
#pragma unroll
            for (int k = 0; k < kGroupsPerWave; k++) {
                const int i0 = first + k * kWave, i = i0 + lane;
                rec[k] = uint4v{0u, 0u, 0u, 0u};
                if (i0 >= n) continue;  // (uniform)
                const int last = min(i0 + kWave, n) - 1;
                SM_SEEK(sw, jl, i0);
                SM_ROUNDS(sw, jl, t, last) {
                    if (i >= sw[t].start && i < sw[t].end) rec[k] = load_record<kStride>(sw[t], i);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kGroupsPerWave; k++) {
            const int i0 = first + k * kWave, i = i0 + lane;
            if (i0 >= n) continue;  // (uniform)
            const int last = min(i0 + kWave, n) - 1;
            int v = 3;  // (no item: i >= n)
            SM_SEEK(sw, j, i0);
            SM_ROUNDS(sw, j, t, last) {
                if (i >= sw[t].start && i < sw[t].end) {
                    float x = __uint_as_float(rec[k].x), y = __uint_as_float(rec[k].y), z = __uint_as_float(rec[k].z);
                    transform(sw[t], x, y, z);
                    v = verdict(gate, x, y, z);
                }
            }
            const unsigned long long keep = __ballot(v == 0);
            if (lane == 0) *as_global(gm + (i0 >> 6)) = keep;
            cnt_nf += (int)__popcll(__ballot(v == 1));
            cnt_or += (int)__popcll(__ballot(v == 2));
        }
    }
    if (lane == 0) {
        wsum[0][wave] = cnt_nf;
        wsum[1][wave] = cnt_or;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int t = 0;
#pragma unroll
        for (int v = 0; v < kBlock / kWave; v++) t += wsum[threadIdx.x][v];
        *as_global(cpre_all + ((size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) + blockIdx.y + 1) * 2 + threadIdx.x) = t;
    }
}

// Kept items of a sequence ahead of item i (0 <= i < n), from the scanned counts and the masks of i's chunk.
__device__ __forceinline__ int kept_ahead(const int* cpre, const unsigned long long* gm, int i) {
    const int c = i / kChunk, g = i >> 6;
    int k = c * kChunk - cpre[2 * c] - cpre[2 * c + 1];
    for (int h = c * kGroupsPerChunk; h < g; h++) k += (int)__popcll(gm[h]);
    return k + (int)__popcll(gm[g] & ((1ull << (i & 63)) - 1ull));
}

// One block per sequence.  Exclusive prefixes over the two chunk counts, in place: cpre[2 c] = items that are not finite
// ahead of chunk c, cpre[2 c + 1] = items out of range ahead of it; the loop carries the sums over any number of chunks
// (up to 8192).  Then tot[j], j < 16: the kept items of sweep j (0 at and beyond n_sweeps) - the kept items ahead of its
// end minus those ahead of its start -, tot[16], tot[17]: the two totals.
__global__ __launch_bounds__(256) void k_sm_scan(const SmSweep* __restrict__ desc, int max_sweeps, int* cpre_all,
                                                long long chunks_per_seq, const unsigned long long* gm_all,
                                                long long groups_per_seq, int* __restrict__ tot_all) {
    __shared__ int wsum[2][256 / kWave];
    __shared__ int ahead[kMaxSweeps + 1];
    const SmSweep* __restrict__ sw = desc + (size_t)blockIdx.x * (size_t)max_sweeps;
    const int n = sw[0].n_items, n_sweeps = sw[0].n_sweeps;
    const int NC = (n + kChunk - 1) / kChunk;
    int* cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) * 2;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    if (tid < 2) cpre[tid] = 0;
    int carry_nf = 0, carry_or = 0;
    for (int c0 = 0; c0 < NC; c0 += 256) {  // (uniform)
        const int c = c0 + tid;
        const IntPair incl = scan_inclusive<kWave>(c < NC ? cpre[2 * (c + 1)] : 0, c < NC ? cpre[2 * (c + 1) + 1] : 0, lane);
        if (lane == kWave - 1) {
            wsum[0][w] = incl.a;
            wsum[1][w] = incl.b;
        }
        __syncthreads();
        int off_nf = carry_nf, off_or = carry_or, total_nf = 0, total_or = 0;
#pragma unroll
        for (int k = 0; k < 256 / kWave; k++) {
            off_nf += k < w ? wsum[0][k] : 0;
            off_or += k < w ? wsum[1][k] : 0;
            total_nf += wsum[0][k];
            total_or += wsum[1][k];
        }
        if (c < NC) {
            cpre[2 * (c + 1)] = off_nf + incl.a;
            cpre[2 * (c + 1) + 1] = off_or + incl.b;
        }
        carry_nf += total_nf;
        carry_or += total_or;
        __syncthreads();  // (also: the prefixes are written before kept_ahead reads them)
    }
    // thread j: the kept items ahead of the start of sweep j; thread n_sweeps: all of them
    if (tid <= n_sweeps) {
        const int i = tid < n_sweeps ? sw[tid].start : n;
        ahead[tid] = i < n ? kept_ahead(cpre, gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq, i) : n - carry_nf - carry_or;
    }
    __syncthreads();
    int* __restrict__ tot = tot_all + (size_t)blockIdx.x * (kMaxSweeps + 2);
    if (tid < kMaxSweeps) tot[tid] = tid < n_sweeps ? ahead[tid + 1] - ahead[tid] : 0;
    if (tid == kMaxSweeps) tot[tid] = carry_nf;
    if (tid == kMaxSweeps + 1) tot[tid] = carry_or;
}

// Grid (sequence, chunk of 1024 items; one block more: the record).  Every wavefront reads the (up to 16) masks of its
// block, one per lane, and scans their counts; the kept lanes of its four groups below the capacity then do the work.
template <int kStride>
__global__ __launch_bounds__(kBlock) void k_sm_write(const SmSweep* __restrict__ desc, int max_sweeps,
                                                    const unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                    const int* __restrict__ cpre_all, long long chunks_per_seq,
                                                    const int* __restrict__ tot_all, long long* __restrict__ record_all) {
    const SmSweep* __restrict__ sw = desc + (size_t)blockIdx.x * (size_t)max_sweeps;
    const int n = sw[0].n_items, capacity = sw[0].capacity;
    const int b = (int)blockIdx.y;
    if (b == (int)gridDim.y - 1) {  // the record, one 8-byte word per thread (include/mld.h: mld_sweep_merge_record)
        const int* __restrict__ tot = tot_all + (size_t)blockIdx.x * (kMaxSweeps + 2);
        const int t = (int)threadIdx.x;
        if (t >= kRecordWords) return;
        const long long n_nf = tot[kMaxSweeps], n_or = tot[kMaxSweeps + 1], n_kept = (long long)n - n_nf - n_or;
        long long word;
        if (t == 0) word = n;
        else if (t == 1) word = n_kept;
        else if (t == 2) word = n_kept < capacity ? n_kept : capacity;
        else if (t == 3) word = n_nf;
        else if (t == 4) word = n_or;
        else if (t < 5 + kMaxSweeps / 2)
            word = (long long)(((unsigned long long)(unsigned)tot[2 * (t - 5) + 1] << 32) | (unsigned)tot[2 * (t - 5)]);
        else word = n_kept > capacity ? MLD_SWEEP_FLAG_TRUNCATED : 0;  // flags, pad_
        *as_global(record_all + (size_t)blockIdx.x * kRecordWords + t) = word;
        return;
    }
    if (b * kChunk >= n) return;  // (uniform in the block)
    const int* __restrict__ cpre = cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1) * 2;
    const int base = b * kChunk - cpre[2 * b] - cpre[2 * b + 1];  // kept items ahead of the chunk
    if (base >= capacity) return;  // nothing of this chunk is stored (uniform in the block)
    const unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = uniform((int)threadIdx.x >> 6);
    const int G = (n + kWave - 1) / kWave;
    const int g_mine = b * kGroupsPerChunk + lane;  // lanes 0..15: the masks of the block
    const unsigned long long mine = (lane < kGroupsPerChunk && g_mine < G) ? gm[g_mine] : 0ull;
    unsigned char* const merged = sw[0].merged;
    MLD_BATCH_GLOBAL uint8_t* sweep_out = as_global(sw[0].sweep_out);
    MLD_BATCH_GLOBAL int32_t* orig_out = as_global(sw[0].orig_out);
    // (the cross-lane reads while every lane is here)
    unsigned lo[kGroupsPerWave], hi[kGroupsPerWave];
    int first_rank[kGroupsPerWave];
    group_ranks<kGroupsPerChunk>(mine, base, lane, wave, lo, hi, first_rank);
    const int first = (b * kGroupsPerChunk + wave * kGroupsPerWave) * kWave;  // the wavefront's first item
    if (first >= n) return;  // (uniform in the wavefront; no cross-lane read below needs the others)
    int j = 0;
    SM_SEEK(sw, j, first);
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave, i = i0 + lane;
        if (i0 >= n) continue;  // (uniform)
        const unsigned long long m = ((unsigned long long)hi[k] << 32) | lo[k];
        if (uniform((int)(m == 0ull || first_rank[k] >= capacity))) continue;  // (every lane holds the group's mask and rank)
        const int rank = first_rank[k] + lane_rank(lo[k], hi[k]);
        const bool mine_set = ((m >> lane) & 1ull) && rank < capacity;  // (a set bit is an item below n)
        const int last = min(i0 + kWave, n) - 1;
        SM_SEEK(sw, j, i0);
        SM_ROUNDS(sw, j, t, last) {
            if (mine_set && i >= sw[t].start && i < sw[t].end) {
                const uint4v r = load_record<kStride>(sw[t], i);
                float x = __uint_as_float(r.x), y = __uint_as_float(r.y), z = __uint_as_float(r.z);
                transform(sw[t], x, y, z);
                const uint4v out = {__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), load_intensity<kStride>(sw[t], i, r.w)};
                *(MLD_BATCH_GLOBAL uint4u*)(merged + (size_t)rank * 16) = out;
                if (sweep_out) sweep_out[rank] = (uint8_t)t;
                if (orig_out) orig_out[rank] = i - sw[t].start;
            }
        }
    }
}

char g_error[512] = "";  // refusals without an object: mld_sweep_merge_last_error(NULL)

}  // namespace

struct mld_sweep_merge : mld_batch::Object {
    int n_seq = 0, max_sweeps = 0;
    int64_t max_points = 0;
    CompactScratch scratch;   // kept mask per group; items not finite and out of range ahead of every chunk (+ the totals)
    DeviceBuffer<int> d_tot;  // per sequence: the kept items of every sweep, the two totals
    mld_batch::DescRing<SmSweep> ring;
};

namespace {

int allocate(mld_sweep_merge* sm) {
    int rc;
    if ((rc = sm->ring.allocate(sm, sm->n_seq * sm->max_sweeps))) return rc;
    if ((rc = sm->d_tot.allocate(sm, (size_t)sm->n_seq * (kMaxSweeps + 2)))) return rc;
    return sm->scratch.allocate(sm, sm->n_seq, (int64_t)sm->max_sweeps * sm->max_points, kChunk, 2);
}

template <int kStride>
void launch_all(mld_sweep_merge* sm, int chunks, SmGate gate, mld_sweep_merge_record* record) {
    const unsigned S = (unsigned)sm->n_seq;
    const CompactScratch& cs = sm->scratch;
    const SmSweep* desc = sm->ring.d_desc.get();
    if (chunks > 0)
        hipLaunchKernelGGL(k_sm_pass<kStride>, dim3(S, (unsigned)chunks), dim3(kBlock), 0, sm->stream, desc, sm->max_sweeps, gate,
                           cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
    hipLaunchKernelGGL(k_sm_scan, dim3(S), dim3(256), 0, sm->stream, desc, sm->max_sweeps, cs.d_cpre.get(), cs.chunks_per_seq,
                       cs.d_gm.get(), cs.groups_per_seq, sm->d_tot.get());
    hipLaunchKernelGGL(k_sm_write<kStride>, dim3(S, (unsigned)chunks + 1u), dim3(kBlock), 0, sm->stream, desc, sm->max_sweeps,
                       cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq, sm->d_tot.get(),
                       reinterpret_cast<long long*>(record));
}

}  // namespace

extern "C" {

mld_sweep_merge* mld_sweep_merge_create(mld_ctx* ctx, int n_seq, int max_sweeps, int64_t max_points, int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_sweep_merge_create: n_seq must be in 1 .. 65536";
        if (max_sweeps < 1 || max_sweeps > kMaxSweeps) return "mld_sweep_merge_create: max_sweeps must be in 1 .. 16";
        if (max_points < 1 || max_points > kMaxPoints) return "mld_sweep_merge_create: max_points must be in 1 .. 8388607";
        if ((int64_t)max_sweeps * max_points > kMaxPoints)
            return "mld_sweep_merge_create: max_sweeps * max_points must be at most 8388607";
        if (!ctx) return "mld_sweep_merge_create: null context";
        return nullptr;
    };
    auto init = [&](mld_sweep_merge* sm) {
        sm->n_seq = n_seq;
        sm->max_sweeps = max_sweeps;
        sm->max_points = max_points;
        return allocate(sm);
    };
    return mld_batch::create_object<mld_sweep_merge>(g_error, "mld_sweep_merge_create", refusal(), ctx, status_out, init);
}

void mld_sweep_merge_destroy(mld_sweep_merge* sm) { mld_batch::destroy_object(sm); }

const char* mld_sweep_merge_last_error(const mld_sweep_merge* sm) { return sm ? sm->err.c_str() : g_error; }

int mld_sweep_merge_run_device(mld_sweep_merge* sm, int n_sweeps, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                               const double* const* T, float min_range, float max_range, const int64_t* capacity,
                               void* const* merged_out, uint8_t* const* sweep_out, int32_t* const* orig_out,
                               mld_sweep_merge_record* record_out_dev) {
    if (!sm) return no_object(g_error, "mld_sweep_merge_run_device", "sm");
#define SM_REFUSE(text) return fail(sm, MLD_ERR_INVALID_ARG, "mld_sweep_merge_run_device: " text)
    if (n_sweeps < 1 || n_sweeps > sm->max_sweeps) SM_REFUSE("n_sweeps must be in 1 .. the max_sweeps of the object");
    if (!pts_dev) SM_REFUSE("null table pts_dev");
    if (!n) SM_REFUSE("null table n");
    if (stride_bytes != 16 && stride_bytes != 32) SM_REFUSE("stride_bytes must be 16 or 32");
    if (!(min_range >= 0.f)) SM_REFUSE("min_range must be >= 0");  // (NaN fails)
    if (!(max_range >= 0.f)) SM_REFUSE("max_range must be >= 0");
    if (min_range > max_range) SM_REFUSE("min_range must not exceed max_range");
    if (!capacity) SM_REFUSE("null table capacity");
    if (!merged_out) SM_REFUSE("null table merged_out");
    if (!record_out_dev) SM_REFUSE("null array record_out_dev");
    if (misaligned(record_out_dev, 7u)) SM_REFUSE("record_out_dev must be 8-byte aligned");
    const int S = sm->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        int64_t items = 0;
        for (int j = 0; j < n_sweeps; j++) {
            const size_t e = (size_t)s * (size_t)n_sweeps + (size_t)j;
            if (n[e] < 0) SM_REFUSE("negative n");
            if (n[e] > sm->max_points)
                return fail(sm, MLD_ERR_CAPACITY, "mld_sweep_merge_run_device: n exceeds the max_points of the object");
            if (n[e] > 0) {
                if (!pts_dev[e]) SM_REFUSE("null array pts_dev of a sweep with points");
                if (misaligned(pts_dev[e], 3u)) SM_REFUSE("pts_dev must be 4-byte aligned");
            }
            items += n[e];
        }
        if (capacity[s] < 0) SM_REFUSE("negative capacity");
        if (items > 0 && capacity[s] > 0) {
            if (!merged_out[s]) SM_REFUSE("null array merged_out of a sequence with points and capacity");
            if (misaligned(merged_out[s], 3u)) SM_REFUSE("merged_out must be 4-byte aligned");
            if (orig_out && orig_out[s] && misaligned(orig_out[s], 3u)) SM_REFUSE("orig_out must be 4-byte aligned");
        }
        if (items > longest) longest = items;  // (<= max_sweeps * max_points <= 8388607)
    }
#undef SM_REFUSE
    for (int s = 0; s < S; s++) {
        SmSweep* q = &sm->ring.stage[(size_t)s * (size_t)sm->max_sweeps];
        int64_t items = 0;
        for (int j = 0; j < n_sweeps; j++) {
            const size_t e = (size_t)s * (size_t)n_sweeps + (size_t)j;
            const double* Tj = T ? T[e] : nullptr;
            q[j] = SmSweep{};
            q[j].cloud = n[e] > 0 ? static_cast<const unsigned char*>(pts_dev[e]) : nullptr;
            q[j].start = (int32_t)items;
            items += n[e];
            q[j].end = (int32_t)items;
            q[j].identity = Tj ? 0 : 1;
            for (int t = 0; t < 12; t++) q[j].T[t] = Tj ? Tj[t] : 0.0;
        }
        const int64_t cap = capacity[s] < items ? capacity[s] : items;
        q[0].n_sweeps = n_sweeps;
        q[0].merged = cap > 0 ? static_cast<unsigned char*>(merged_out[s]) : nullptr;
        q[0].sweep_out = (cap > 0 && sweep_out) ? sweep_out[s] : nullptr;
        q[0].orig_out = (cap > 0 && orig_out) ? orig_out[s] : nullptr;
        q[0].n_items = (int32_t)items;
        q[0].capacity = (int32_t)cap;
    }
    const SmGate gate = {min_range * min_range, max_range * max_range};
    MLD_HIP(sm, hipSetDevice(sm->device));
    const int rc = sm->ring.upload(sm);
    if (rc) return rc;
    const int chunks = (int)((longest + kChunk - 1) / kChunk);  // (<= 8192)
    with_stride(stride_bytes, [&](auto stride) { launch_all<decltype(stride)::value>(sm, chunks, gate, record_out_dev); });
    MLD_HIP(sm, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
