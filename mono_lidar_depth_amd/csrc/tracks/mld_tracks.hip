// mld_tracks.hip — the device-resident tracklet store of the batched tracklet layer (include/mld.h, "mld_tracks").
//
// TrackletDepthModule keeps `_trackletMap`, a std::map<int, Tracklet> whose values are deques of (u, v, depth)
// (tracklets_depth/src/tracklet_depth_module.cpp): ExractNewTrackletFrames asks it which ids are new (:23-61),
// SaveFeatureDepths pushes this frame's features to the front (:119-169), TidyUpTracklets erases every track without
// an update (:171-193), convert_tracklets_to_matches_msg reads the tracks back in message order (:209-259).  Here the
// map of every sequence lives in GPU memory and those four steps are kernels over all sequences at once.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream, mld_last_error,
// mld_tracklets_depths_device); it shares no internals with mld_api.hip.  Descriptor ring and object skeleton:
// ../batch/mld_batch_object.h.
//
// Data, per sequence (everything allocated in mld_tracks_create):
//   table[2][cap]      open-addressed id tables, cap = power of two >= 2 * max_tracks, linear probing.  A slot is
//                      64 bits: bit 63 = occupied, bits 32..62 = history row, bits 0..31 = the id.  0 is "empty", so
//                      every int32 is a legal id.  One table holds the last committed frame, the other is empty and
//                      receives the next frame: a frame's live set is exactly its ids, so nothing is ever deleted
//                      from a table that is probed (no tombstones).
//   hist[max_tracks][max_history][3]   history rows, ring buffers of (float(int u), float(int v), d), with
//   head[], len[]      the position of the newest entry and the number of stored entries of every row
//   mark[]             the epoch (frame counter) of the last look-up that found the row's track
//   free_rows[], top   the pool: a stack of unused rows
//   row/slot/dup_row[2][max_tracks]    per track of the last committed / the pending frame: its row, its table slot
//                      (-1: a repeated id that lost), and a row taken for a repeated id that has to go back to the pool
//
// Kernels, one launch over all sequences each (flat grid, block -> (sequence, chunk) through the block prefix in the
// descriptors), ordered by kernel boundaries only:
//   k_tracks_lookup    begin:  probe the committed table, write is_new and the row, stamp mark[row] = epoch
//   k_tracks_release   commit: every track of the committed frame clears its slot (the table is empty afterwards) and,
//                      if this frame did not stamp its row, pushes the row on the pool; clears the frame counters
//   k_tracks_commit    commit: one thread per track: a new track pops a row, the track claims a slot of the other
//                      table with atomicCAS, then pushes its entries
//   k_tracks_export / k_tracks_count   read-only
//   k_tracks_pack_sums / _scan / _write   read-only: the packed export, tracks back to back with offsets (below)
//   k_tracks_leave_sums / _scan / _write  read-only, between a look-up and its commit: the tracks that commit erases and
//                      the entries it overwrites (at the kernels)
//   k_tracks_reset / k_tracks_import      the packed import, the inverse of that export, for selected sequences: the
//                      committed table and the pool as created, then insert + fill (at the kernels); the reset alone
//                      empties sequences (mld_tracks_reset_device, the restart of mld_tracklets_step_lanes_device)
//   k_tracks_no_previous   a lanes step with mixed flags: d_last = -1 for the new tracks of the sequences without a
//                      previous frame, which the depth call saw with an all-zero mask (at mld_tracklets_step_lanes_device)
// Rows are released before they are taken and never in the same kernel, so max_tracks rows per sequence sustain
// max_tracks tracks per frame at any churn, and the stack needs no ABA care.
//
// The packed export (mld_tracks_export_packed_device) is a segmented exclusive scan of the tracks' lengths followed by
// a compaction, three kernels over the same flat (sequence, chunk of 256 tracks) blocks, no block ever waiting on
// another (no look-back, no flags):
//   k_tracks_pack_sums   block b: the sum of its 256 lengths (wave64 reduction) -> pack_sum[b] (32 bits: at most
//                        256 * 65535); every track's length and ring head, gathered through its row here, are left in
//                        pack_meta in track order so that the third pass reads them coalesced
//   k_tracks_pack_scan   one block per sequence: exclusive scan of the sequence's block sums, kScanWidth at a time with
//                        a 64-bit carry -> pack_base[b]
//   k_tracks_pack_write  block b: rescans its 256 lengths (pack_meta) into LDS, writes offsets[i] = pack_base[b] + the local
//                        prefix (the last block of a sequence adds offsets[n]), then walks its own contiguous output
//                        range below the capacity with one thread per entry - the owning track by a binary search in
//                        the LDS prefix, the ring position as k_tracks_export - so that the 12-byte entries leave as
//                        contiguous runs.
//   pack_sum / pack_base hold one entry per possible block, n_seq * ceil(max_tracks / 256), pack_meta one 32-bit word
//   per track (length | head << 16: both are below 65536); allocated at create.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../batch/mld_batch_object.h"

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kOccupied = 1ull << 63;

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing), read by every kernel
// of the call.
struct TrSeq {
    union {
        const int32_t* ids;
        int32_t* ids_out;  // mld_tracks_export_leaving_device (as every second member of the unions down to u_old)
    };
    union {
        uint8_t* is_new;
        int32_t* spill_ids_out;
    };
    union {
        const float* u_new;
        float* spill_fp_out;
    };
    union {
        const float* v_new;
        int64_t track_capacity;  // tracks ids_out holds; offsets_out holds one more entry
    };
    union {
        const float* u_old;
        int64_t spill_capacity;  // entries spill_ids_out / spill_fp_out hold
    };
    const float* v_old;
    const float* d_cur;
    union {
        const float* d_last;
        float* d_last_w;    // mld_tracklets_step_lanes_device: d_last_out of a sequence without a previous frame
        int64_t capacity;   // mld_tracks_export_packed_device, mld_tracks_export_leaving_device: entries fp_out holds
        int64_t n_entries;  // mld_tracks_import_packed_device: entries fp_in holds
    };
    union {
        float* fp_out;
        const float* fp_in;  // mld_tracks_import_packed_device
    };
    union {
        int32_t* len_out;           // mld_tracks_export_device (k_tracks_no_previous: type_last_out)
        int64_t* offsets_out;       // mld_tracks_export_packed_device
        const int64_t* offsets_in;  // mld_tracks_import_packed_device
    };
    int32_t n;          // tracks of the frame the call works on
    union {
        int32_t n_prev;      // tracks of the committed frame (release pass)
        int32_t leave_mode;  // mld_tracks_export_leaving_device: kLeaveSkip / kLeaveMarks / kLeaveFlush
    };
    int32_t blk0;       // first block of the sequence in a launch over n (export: over n * max_history)
    int32_t blk0_prev;  // the same for the release pass (at least one block per sequence; reset: over the table's
                        // slots, and none for a sequence that is not selected)
};
static_assert(sizeof(TrSeq) == 96, "96 bytes per sequence (DESIGN.md)");

struct TrDev {
    unsigned long long* table;  // [2][n_seq][cap]
    float* hist;                // [n_seq][M][H][3]
    int32_t* head;              // [n_seq][M]
    int32_t* len;               // [n_seq][M]
    uint32_t* mark;             // [n_seq][M]
    int32_t* free_rows;         // [n_seq][M]
    int32_t* top;               // [n_seq]
    int32_t* row;               // [2][n_seq][M]
    int32_t* slot;              // [2][n_seq][M]
    int32_t* dup_row;           // [2][n_seq][M]
    unsigned int* cnt;          // [n_seq][4]: new, old, repeated ids, tracks dropped for want of a row (never)
    unsigned long long* feat;   // [n_seq][2]: stored features with d >= 0, the others
    uint32_t* pack_sum;         // [n_seq * ceil(M / 256)]: packed export, the entries of every block of 256 tracks
    unsigned long long* pack_base;  // the same blocks: entries of the sequence in front of the block
    uint32_t* pack_meta;        // [n_seq][M]: packed export, length | head << 16 of every track of the committed frame
    int32_t n_seq, M, H;
    uint32_t cap;
};

__device__ __forceinline__ uint32_t hash_id(int32_t id) {  // (murmur3's finaliser)
    uint32_t h = (uint32_t)id;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// The sequence a block belongs to: the last one whose first block is <= b (sequences without blocks share their
// successor's first block and are skipped).
template <bool kPrev>
__device__ __forceinline__ int seq_of_block(const TrSeq* __restrict__ desc, int n_seq, int b) {
    int lo = 0, hi = n_seq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((kPrev ? desc[mid].blk0_prev : desc[mid].blk0) <= b) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ void wave_count(unsigned int* dst, bool pred) {
    const unsigned long long m = __ballot(pred);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(dst, (unsigned int)__popcll(m));
}

__global__ __launch_bounds__(256) void k_tracks_init(TrDev T) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)T.n_seq * T.M;
    if (i < total) T.free_rows[i] = (int32_t)(i % (size_t)T.M);
    if (i < (size_t)T.n_seq) T.top[i] = T.M;
}

// ExractNewTrackletFrames' `_trackletMap.count(id)` (:31) for every track of every sequence.
__global__ __launch_bounds__(kBlock) void k_tracks_lookup(TrDev T, const TrSeq* __restrict__ desc, int prev, uint32_t epoch) {
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + (int)threadIdx.x;
    if (i >= q.n) return;
    const int32_t id = q.ids[i];
    const unsigned long long* __restrict__ tab = T.table + ((size_t)prev * T.n_seq + s) * T.cap;
    const uint32_t mask = T.cap - 1;
    uint32_t h = hash_id(id) & mask;
    int row = -1;
    for (uint32_t k = 0; k < T.cap; k++) {  // (the table is at most half full: an empty slot ends every chain)
        const unsigned long long e = tab[h];
        if (!(e & kOccupied)) break;
        if ((uint32_t)e == (uint32_t)id) {
            row = (int)((e >> 32) & 0x7fffffffu);
            break;
        }
        h = (h + 1) & mask;
    }
    const size_t base = (size_t)s * T.M;
    if (row >= 0) T.mark[base + row] = epoch;
    T.row[((size_t)(1 - prev) * T.n_seq + s) * T.M + i] = row;
    q.is_new[i] = row < 0 ? 1 : 0;
}

// A row back on the sequence's free stack.  (The stack cannot overflow - every row is released once; the test keeps a
// miscount from ever becoming a store outside the array.)
__device__ __forceinline__ void free_row(const TrDev& T, int s, int row) {
    const int p = atomicAdd(&T.top[s], 1);
    if (p >= 0 && p < T.M) T.free_rows[(size_t)s * T.M + p] = row;
}

// TidyUpTracklets (:171-193): the rows of the committed frame's tracks that the pending frame did not find go back to
// the pool; the committed table is emptied slot by slot (its tracks know their slots).
__global__ __launch_bounds__(kBlock) void k_tracks_release(TrDev T, const TrSeq* __restrict__ desc, int prev, uint32_t epoch) {
    const int s = seq_of_block<true>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0_prev) * kBlock + (int)threadIdx.x;
    if (i < 4 && (int)blockIdx.x == q.blk0_prev) T.cnt[(size_t)s * 4 + i] = 0;
    if (i >= q.n_prev) return;
    const size_t ps = ((size_t)prev * T.n_seq + s) * T.M + i;
    const size_t base = (size_t)s * T.M;
    const int slot = T.slot[ps], row = T.row[ps], dup_row = T.dup_row[ps];
    if (slot >= 0) {
        T.table[((size_t)prev * T.n_seq + s) * T.cap + slot] = 0ull;
        if (T.mark[base + row] != epoch) free_row(T, s, row);
    }
    if (dup_row >= 0) free_row(T, s, dup_row);
}

__device__ __forceinline__ void push_front(float* __restrict__ hr, int H, int& head, int& len, float u, float v, float d) {
    head = head == 0 ? H - 1 : head - 1;
    hr[head * 3 + 0] = u;
    hr[head * 3 + 1] = v;
    hr[head * 3 + 2] = d;
    len = len < H ? len + 1 : H;
}

// SaveFeatureDepths (:119-169) into the table of the pending frame.
__global__ __launch_bounds__(kBlock) void k_tracks_commit(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + (int)threadIdx.x;
    bool made = false, updated = false, repeated = false, dropped = false;
    if (i < q.n) {
        const size_t ps = ((size_t)cur * T.n_seq + s) * T.M + i;
        const size_t base = (size_t)s * T.M;
        int row = T.row[ps];
        const bool fresh = row < 0;
        if (fresh) {
            const int t = atomicSub(&T.top[s], 1);
            if (t > 0 && t <= T.M) {
                row = T.free_rows[base + t - 1];
            } else {  // (cannot happen: rows were released before, and n <= max_tracks)
                atomicAdd(&T.top[s], 1);
                dropped = true;
            }
        }
        int slot = -1, dup_row = -1;
        if (!dropped) {
            const int32_t id = q.ids[i];
            const unsigned long long mine = kOccupied | ((unsigned long long)(uint32_t)row << 32) | (uint32_t)id;
            unsigned long long* tab = T.table + ((size_t)cur * T.n_seq + s) * T.cap;
            const uint32_t mask = T.cap - 1;
            uint32_t h = hash_id(id) & mask;
            for (uint32_t k = 0; k < T.cap; k++) {
                const unsigned long long old = atomicCAS(&tab[h], 0ull, mine);
                if (old == 0ull) {
                    slot = (int)h;
                    break;
                }
                if ((uint32_t)old == (uint32_t)id) {  // the id occurs twice in this frame: the first claim stays
                    repeated = true;
                    if (fresh) dup_row = row;
                    row = (int)((old >> 32) & 0x7fffffffu);
                    break;
                }
                h = (h + 1) & mask;
            }
            if (slot < 0 && !repeated) {  // (a full table: cannot happen, cap >= 2 * max_tracks)
                dropped = true;
                if (fresh) dup_row = row;
            }
        }
        if (slot >= 0) {
            float* hr = T.hist + (base + row) * (size_t)T.H * 3;
            int head = 0, len = 0;
            if (fresh) {  // a new tracklet starts with the previous feature (:134-151)
                push_front(hr, T.H, head, len, (float)(int)q.u_old[i], (float)(int)q.v_old[i], q.d_last[i]);
                made = true;
            } else {
                head = T.head[base + row];
                len = T.len[base + row];
                updated = true;
            }
            push_front(hr, T.H, head, len, (float)(int)q.u_new[i], (float)(int)q.v_new[i], q.d_cur[i]);
            T.head[base + row] = head;
            T.len[base + row] = len;
        }
        T.row[ps] = dropped ? -1 : row;
        T.slot[ps] = slot;
        T.dup_row[ps] = dup_row;
    }
    unsigned int* cnt = T.cnt + (size_t)s * 4;
    wave_count(cnt + 0, made);
    wave_count(cnt + 1, updated);
    wave_count(cnt + 2, repeated);
    wave_count(cnt + 3, dropped);
}

// convert_tracklets_to_matches_msg (:209-259): one thread per (track, history position).
__global__ __launch_bounds__(kBlock) void k_tracks_export(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const long long idx = ((long long)blockIdx.x - q.blk0) * kBlock + threadIdx.x;
    const long long i = idx / T.H;
    const int h = (int)(idx - i * T.H);
    if (i >= q.n) return;
    const size_t base = (size_t)s * T.M;
    const int row = T.row[((size_t)cur * T.n_seq + s) * T.M + (size_t)i];
    const int len = row >= 0 ? T.len[base + row] : 0;
    if (h == 0 && q.len_out) q.len_out[i] = len;
    if (h >= len || !q.fp_out) return;
    int p = T.head[base + row] + h;
    if (p >= T.H) p -= T.H;
    const float* __restrict__ src = T.hist + ((base + row) * (size_t)T.H + p) * 3;
    float* dst = q.fp_out + (size_t)idx * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

// The (success, failed) pair of convert_tracklets_to_matches_msg (:235): stored features with depth >= 0 / the others.
__global__ __launch_bounds__(kBlock) void k_tracks_count(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + (int)threadIdx.x;
    unsigned int good = 0, bad = 0;
    if (i < q.n) {
        const size_t ps = ((size_t)cur * T.n_seq + s) * T.M + i;
        const size_t base = (size_t)s * T.M;
        if (T.slot[ps] >= 0) {  // (a repeated id counts once)
            const int row = T.row[ps];
            const int len = T.len[base + row];
            const float* __restrict__ hr = T.hist + (base + row) * (size_t)T.H * 3;
            const int head = T.head[base + row];
            for (int k = 0; k < len; k++) {
                int p = head + k;
                if (p >= T.H) p -= T.H;
                if (hr[p * 3 + 2] >= 0.0f) good++; else bad++;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        good += __shfl_down(good, off);
        bad += __shfl_down(bad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (good) atomicAdd(&T.feat[(size_t)s * 2 + 0], (unsigned long long)good);
        if (bad) atomicAdd(&T.feat[(size_t)s * 2 + 1], (unsigned long long)bad);
    }
}

// ---- the packed export ----
constexpr int kScanWidth = 256;  // block sums one pass of k_tracks_pack_scan takes (its block size)


// Exclusive prefix of one value per thread over the 256 threads of a block; *total = the sum, in every thread.
template <typename V>
__device__ __forceinline__ V block_scan_exclusive(V v, V* s_wave, V* total) {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    V inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const V up = __shfl_up(inc, off);
        if (lane >= off) inc += up;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    V before = 0, all = 0;
    for (int k = 0; k < kBlock / 64; k++) {
        const V t = s_wave[k];
        if (k < w) before += t;
        all += t;
    }
    __syncthreads();  // (s_wave is free for the caller's next scan)
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kBlock) void k_tracks_pack_sums(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + (int)threadIdx.x;
    uint32_t sum = 0;
    if (i < q.n) {  // (a repeated id that lost has the stored occurrence's row: it exports that history)
        const size_t base = (size_t)s * T.M;
        const int row = T.row[((size_t)cur * T.n_seq + s) * T.M + (size_t)i];
        sum = row >= 0 ? (uint32_t)T.len[base + row] : 0u;
        const uint32_t head = sum ? (uint32_t)T.head[base + row] : 0u;
        T.pack_meta[base + i] = sum | (head << 16);  // (max_history <= 65535)
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (int k = 0; k < kBlock / 64; k++) all += s_wave[k];
        T.pack_sum[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kScanWidth) void k_tracks_pack_scan(TrDev T, const TrSeq* __restrict__ desc) {
    static_assert(kScanWidth == kBlock, "block_scan_exclusive scans kBlock threads");
    __shared__ unsigned long long s_wave[kBlock / 64];
    const TrSeq& q = desc[blockIdx.x];
    const int nb = (q.n + kBlock - 1) / kBlock;  // (uniform over the block: every thread takes every pass)
    unsigned long long carry = 0;
    for (int j0 = 0; j0 < nb; j0 += kScanWidth) {
        const int j = j0 + (int)threadIdx.x;
        const unsigned long long v = j < nb ? (unsigned long long)T.pack_sum[q.blk0 + j] : 0ull;
        unsigned long long all;
        const unsigned long long before = block_scan_exclusive(v, s_wave, &all);
        if (j < nb) T.pack_base[q.blk0 + j] = carry + before;
        carry += all;
    }
}

__global__ __launch_bounds__(kBlock) void k_tracks_pack_write(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    __shared__ uint32_t s_wave[kBlock / 64];
    __shared__ uint32_t s_off[kBlock + 1];
    __shared__ int32_t s_row[kBlock], s_head[kBlock];
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int t = (int)threadIdx.x;
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + t;
    const size_t base = (size_t)s * T.M;
    const uint32_t meta = i < q.n ? T.pack_meta[base + i] : 0u;
    const uint32_t len = meta & 0xffffu;
    uint32_t total;
    const uint32_t before = block_scan_exclusive(len, s_wave, &total);
    const long long first = (long long)T.pack_base[blockIdx.x];  // entries of the sequence in front of this block
    s_off[t] = before;
    s_row[t] = len ? T.row[((size_t)cur * T.n_seq + s) * T.M + (size_t)i] : -1;
    s_head[t] = (int32_t)(meta >> 16);
    if (t == 0) s_off[kBlock] = total;
    if (i < q.n) q.offsets_out[i] = first + (long long)before;
    if (i == q.n - 1) q.offsets_out[q.n] = first + (long long)total;
    __syncthreads();
    const long long room = (long long)q.capacity - first;  // entries of this block's range below the capacity
    if (!q.fp_out || room <= 0) return;
    const uint32_t limit = room < (long long)total ? (uint32_t)room : total;
    float* __restrict__ dst0 = q.fp_out + (size_t)first * 3;
    for (uint32_t e = (uint32_t)t; e < limit; e += kBlock) {
        int lo = 0, hi = kBlock;  // the last track whose prefix is <= e: tracks without entries in front of it are passed
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= e) lo = mid; else hi = mid;
        }
        int p = s_head[lo] + (int)(e - s_off[lo]);
        if (p >= T.H) p -= T.H;
        const float* __restrict__ src = T.hist + ((base + s_row[lo]) * (size_t)T.H + p) * 3;
        float* dst = dst0 + (size_t)e * 3;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
    }
}

// ---- the leaving export: what the commit of the begun frame removes from the store ----
//
// Between a look-up and its commit, of every stored track of the committed frame (slot >= 0):
//   ended    mark != epoch (or the sequence is flushed): k_tracks_release hands its row back; id, offset and entries go
//            out as the packed export writes them
//   spilled  mark == epoch and len == max_history: k_tracks_commit's push_front overwrites the oldest entry, ring
//            position head + H - 1; id and that entry go out
// The packed export's three kernels with three columns (ended tracks, their entries, spilled tracks) in place of one,
// on the same flat (sequence, chunk of 256 committed tracks) blocks and in the same scratch (the store serves one call
// at a time):
//   pack_meta[track]  ended: length | head << 16;  spilled: kLeaveSpill | the oldest entry's ring position;  neither:
//                     kLeaveNone.  (head and ring positions are below max_history <= 65535: the upper half 0xffff is
//                     no head.)
//   pack_base[block]  sums -> scan: ended | spilled << 10 | entries << 20 (at most 256, 256 and 256 * 65535)
//                     scan -> write: entries of the sequence in front of the block (40 bits: below 2^24 * 65535) |
//                     ended tracks in front of it << 40 (below max_tracks <= 2^24)
//   pack_sum[block]   scan -> write: spilled tracks of the sequence in front of the block
// No atomics: the order of both streams is the committed frame's.  No block waits on another.
constexpr uint32_t kLeaveNone = 0xffffffffu;
constexpr uint32_t kLeaveSpill = 0xffff0000u;
constexpr int kLeaveSkip = 0, kLeaveMarks = 1, kLeaveFlush = 2;  // TrSeq::leave_mode (skip: n = 0, the record stays)

__global__ __launch_bounds__(kBlock) void k_tracks_leave_sums(TrDev T, const TrSeq* __restrict__ desc, int cur, uint32_t epoch) {
    __shared__ unsigned long long s_wave[kBlock / 64];
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + (int)threadIdx.x;
    unsigned long long sum = 0;
    if (i < q.n) {
        const size_t ps = ((size_t)cur * T.n_seq + s) * T.M + (size_t)i;
        const size_t base = (size_t)s * T.M;
        uint32_t meta = kLeaveNone;
        if (T.slot[ps] >= 0) {  // (a repeated id that lost: the stored occurrence stands for it)
            const int row = T.row[ps];
            const uint32_t len = (uint32_t)T.len[base + row], head = (uint32_t)T.head[base + row];
            if (q.leave_mode == kLeaveFlush || T.mark[base + row] != epoch) {
                meta = len | (head << 16);
                sum = 1ull | ((unsigned long long)len << 20);
            } else if (len == (uint32_t)T.H) {
                uint32_t oldest = head + (uint32_t)T.H - 1u;
                if (oldest >= (uint32_t)T.H) oldest -= (uint32_t)T.H;
                meta = kLeaveSpill | oldest;
                sum = 1ull << 10;
            }
        }
        T.pack_meta[base + i] = meta;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int k = 0; k < kBlock / 64; k++) all += s_wave[k];
        T.pack_base[blockIdx.x] = all;
    }
}

// One block per sequence, as k_tracks_pack_scan; the totals are the sequence's record (three int64 and a zero).
__global__ __launch_bounds__(kScanWidth) void k_tracks_leave_scan(TrDev T, const TrSeq* __restrict__ desc, long long* __restrict__ record) {
    __shared__ unsigned long long s_wave[kBlock / 64];
    const TrSeq& q = desc[blockIdx.x];
    if (q.leave_mode == kLeaveSkip) return;  // (uniform over the block)
    const int nb = (q.n + kBlock - 1) / kBlock;
    unsigned long long carry_ts = 0, carry_e = 0;  // ended tracks | spilled tracks << 32 (both <= 2^24); entries
    for (int j0 = 0; j0 < nb; j0 += kScanWidth) {
        const int j = j0 + (int)threadIdx.x;
        const unsigned long long v = j < nb ? T.pack_base[q.blk0 + j] : 0ull;
        unsigned long long all_ts, all_e;
        const unsigned long long before_ts = block_scan_exclusive((v & 0x3ffull) | (((v >> 10) & 0x3ffull) << 32), s_wave, &all_ts);
        const unsigned long long before_e = block_scan_exclusive(v >> 20, s_wave, &all_e);
        if (j < nb) {
            const unsigned long long ts = carry_ts + before_ts;
            T.pack_base[q.blk0 + j] = (carry_e + before_e) | ((ts & 0xffffffffull) << 40);
            T.pack_sum[q.blk0 + j] = (uint32_t)(ts >> 32);
        }
        carry_ts += all_ts;
        carry_e += all_e;
    }
    if (threadIdx.x == 0) {
        long long* r = record + (size_t)blockIdx.x * 4;
        r[0] = (long long)(carry_ts & 0xffffffffull);
        r[1] = (long long)carry_e;
        r[2] = (long long)(carry_ts >> 32);
        r[3] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_tracks_leave_write(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    __shared__ uint32_t s_wave[kBlock / 64];
    __shared__ uint32_t s_off[kBlock + 1];
    __shared__ int32_t s_row[kBlock], s_head[kBlock];
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int t = (int)threadIdx.x;
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + t;
    const size_t base = (size_t)s * T.M;
    const uint32_t meta = i < q.n ? T.pack_meta[base + i] : kLeaveNone;
    const bool ended = (meta >> 16) != 0xffffu, spilled = !ended && meta != kLeaveNone;
    const uint32_t len = ended ? (meta & 0xffffu) : 0u;
    uint32_t n_flags, total;
    const uint32_t flags_before = block_scan_exclusive((ended ? 1u : 0u) | (spilled ? 1u << 16 : 0u), s_wave, &n_flags);
    const uint32_t before = block_scan_exclusive(len, s_wave, &total);
    const unsigned long long pb = T.pack_base[blockIdx.x];
    const long long first = (long long)(pb & ((1ull << 40) - 1));  // entries of the sequence's ended tracks in front of this block
    const long long first_track = (long long)(pb >> 40);
    const long long first_spill = (long long)T.pack_sum[blockIdx.x];
    int row = -1;
    int32_t id = 0;
    if (ended || spilled) {
        const size_t ps = ((size_t)cur * T.n_seq + s) * T.M + (size_t)i;
        row = T.row[ps];
        id = (int32_t)(uint32_t)T.table[((size_t)cur * T.n_seq + s) * T.cap + (size_t)T.slot[ps]];
    }
    s_off[t] = before;
    s_row[t] = len ? row : -1;
    s_head[t] = (int32_t)(meta >> 16);
    if (t == 0) s_off[kBlock] = total;
    const long long track_cap = (long long)q.track_capacity;
    if (ended) {
        const long long k = first_track + (long long)(flags_before & 0xffffu);
        if (k < track_cap) q.ids_out[k] = id;
        if (k <= track_cap && track_cap > 0) q.offsets_out[k] = first + (long long)before;  // (k == capacity: the closing entry)
    }
    if (t == 0 && (int)blockIdx.x - q.blk0 == (q.n - 1) / kBlock) {  // the closing entry of a sequence that is not truncated
        const long long n_ended = first_track + (long long)(n_flags & 0xffffu);
        if (n_ended <= track_cap && track_cap > 0) q.offsets_out[n_ended] = first + (long long)total;
    }
    if (spilled) {
        const long long k = first_spill + (long long)(flags_before >> 16);
        if (k < (long long)q.spill_capacity) {
            q.spill_ids_out[k] = id;
            const float* __restrict__ src = T.hist + ((base + row) * (size_t)T.H + (meta & 0xffffu)) * 3;
            float* dst = q.spill_fp_out + (size_t)k * 3;
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
        }
    }
    __syncthreads();
    const long long room = (long long)q.capacity - first;  // entries of this block's range below the capacity
    if (!q.fp_out || room <= 0) return;
    const uint32_t limit = room < (long long)total ? (uint32_t)room : total;
    float* __restrict__ dst0 = q.fp_out + (size_t)first * 3;
    for (uint32_t e = (uint32_t)t; e < limit; e += kBlock) {
        int lo = 0, hi = kBlock;  // the last track whose prefix is <= e (k_tracks_pack_write)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= e) lo = mid; else hi = mid;
        }
        int p = s_head[lo] + (int)(e - s_off[lo]);
        if (p >= T.H) p -= T.H;
        const float* __restrict__ src = T.hist + ((base + s_row[lo]) * (size_t)T.H + p) * 3;
        float* dst = dst0 + (size_t)e * 3;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
    }
}

// ---- the packed import: the inverse of the packed export ----

// The selected sequences as mld_tracks_create left them: the committed table without an id, every row on the free stack
// (free_rows[p] = p, top = max_tracks), the frame counters at zero.  Flat over (selected sequence, 256 table slots) -
// cap >= max_tracks, so the same index walks the stack.  Independent of what the sequence held; the other table is
// empty already (the store's invariant).
__global__ __launch_bounds__(kBlock) void k_tracks_reset(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    const int s = seq_of_block<true>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const uint32_t j = (uint32_t)((int)blockIdx.x - q.blk0_prev) * kBlock + threadIdx.x;
    if (j >= T.cap) return;
    T.table[((size_t)cur * T.n_seq + s) * T.cap + j] = 0ull;
    if (j < (uint32_t)T.M) T.free_rows[(size_t)s * T.M + j] = (int32_t)j;
    if (j < 4) T.cnt[(size_t)s * 4 + j] = 0;
    if (j == 0) T.top[s] = T.M;
}

// Insert and fill in one kernel over blocks of 256 tracks of the selected sequences (after k_tracks_reset).
//   insert  one thread per track.  The pool is as created, so the n pops are known without atomics: track i takes
//           free_rows[M - 1 - i] = row M - 1 - i and thread 0 leaves top = M - n.  The slot is claimed in the COMMITTED
//           table as k_tracks_commit claims it; a repeated id that lost keeps slot -1, the winner's row and its own row
//           in dup_row (the next commit's k_tracks_release walks row / slot / dup_row of every i < n and hands it back).
//           Offsets are clamped to [0, n_entries]; a decreasing pair is a track without entries; head = 0,
//           len = min(L, H): the newest entries stay.
//   fill    the mirror of k_tracks_pack_write: the stored lengths (0 for a loser) are prefix-summed in LDS, one thread
//           per entry finds its track by binary search and moves 12 bytes from the track's run to its row - runs of
//           consecutive tracks are consecutive in fp_in wherever an export wrote them.  A thread knows whether its track
//           won as soon as its own atomicCAS returns, so the fill needs no second kernel.
__global__ __launch_bounds__(kBlock) void k_tracks_import(TrDev T, const TrSeq* __restrict__ desc, int cur) {
    __shared__ uint32_t s_wave[kBlock / 64];
    __shared__ uint32_t s_off[kBlock + 1];
    __shared__ int32_t s_row[kBlock];
    __shared__ long long s_src[kBlock];
    const int s = seq_of_block<false>(desc, T.n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int t = (int)threadIdx.x;
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + t;
    const size_t base = (size_t)s * T.M;
    bool made = false, repeated = false;
    uint32_t len = 0;
    long long src0 = 0;
    int row = -1;
    if (i < q.n) {
        const long long E = (long long)q.n_entries;
        long long o0 = q.offsets_in[i], o1 = q.offsets_in[i + 1];
        o0 = o0 < 0 ? 0 : (o0 > E ? E : o0);
        o1 = o1 < 0 ? 0 : (o1 > E ? E : o1);
        const long long L = o1 > o0 ? o1 - o0 : 0;
        src0 = o0;
        row = T.M - 1 - i;
        if (i == 0) T.top[s] = T.M - q.n;
        const int32_t id = q.ids[i];
        const unsigned long long mine = kOccupied | ((unsigned long long)(uint32_t)row << 32) | (uint32_t)id;
        unsigned long long* tab = T.table + ((size_t)cur * T.n_seq + s) * T.cap;
        const uint32_t mask = T.cap - 1;
        uint32_t h = hash_id(id) & mask;
        int slot = -1, dup_row = -1;
        for (uint32_t k = 0; k < T.cap; k++) {
            const unsigned long long old = atomicCAS(&tab[h], 0ull, mine);
            if (old == 0ull) {
                slot = (int)h;
                break;
            }
            if ((uint32_t)old == (uint32_t)id) {  // the id occurs twice: the first claim stays
                repeated = true;
                dup_row = row;
                row = (int)((old >> 32) & 0x7fffffffu);
                break;
            }
            h = (h + 1) & mask;
        }
        if (slot < 0 && !repeated) {  // (a full table: cannot happen, cap >= 2 * max_tracks)
            dup_row = row;
            row = -1;
        }
        if (slot >= 0) {
            len = (uint32_t)(L < (long long)T.H ? L : (long long)T.H);
            T.head[base + row] = 0;
            T.len[base + row] = (int32_t)len;
            made = true;
        }
        const size_t ps = ((size_t)cur * T.n_seq + s) * T.M + i;
        T.row[ps] = row;
        T.slot[ps] = slot;
        T.dup_row[ps] = dup_row;
    }
    unsigned int* cnt = T.cnt + (size_t)s * 4;
    wave_count(cnt + 0, made);
    wave_count(cnt + 2, repeated);
    uint32_t total;
    const uint32_t before = block_scan_exclusive(len, s_wave, &total);
    s_off[t] = before;
    s_row[t] = row;
    s_src[t] = src0;
    if (t == 0) s_off[kBlock] = total;
    __syncthreads();
    for (uint32_t e = (uint32_t)t; e < total; e += kBlock) {
        int lo = 0, hi = kBlock;  // the last track whose prefix is <= e (k_tracks_pack_write)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= e) lo = mid; else hi = mid;
        }
        const uint32_t k = e - s_off[lo];  // (k < the track's stored length <= H; src0 + k < n_entries)
        const float* __restrict__ src = q.fp_in + (size_t)(s_src[lo] + (long long)k) * 3;
        float* dst = T.hist + ((base + s_row[lo]) * (size_t)T.H + k) * 3;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
    }
}

// The new tracks of the sequences of a lanes step that have no previous frame: d_last = -1, type_last =
// MLD_Unspecified - what the depth call answers without a previous cloud (tracklet_depth_module.cpp:93-96).  The depth
// call saw an all-zero mask for these sequences, so it evaluated none of their previous features and wrote neither array.
__global__ __launch_bounds__(kBlock) void k_tracks_no_previous(const TrSeq* __restrict__ desc, int n_seq) {
    const int s = seq_of_block<false>(desc, n_seq, (int)blockIdx.x);
    const TrSeq& q = desc[s];
    const int i = ((int)blockIdx.x - q.blk0) * kBlock + (int)threadIdx.x;
    if (i >= q.n || !q.is_new[i]) return;
    q.d_last_w[i] = -1.0f;
    if (q.len_out) q.len_out[i] = (int32_t)MLD_Unspecified;
}

char g_create_error[512] = "";

// The output arguments of mld_tracks_export_leaving_device: host tables of n_seq entries, one record array on the device.
struct LeaveOut {
    int32_t* const* ids_out;
    int64_t* const* offsets_out;
    float* const* fp_out;
    int32_t* const* spill_ids_out;
    float* const* spill_fp_out;
    const int64_t* track_capacity;
    const int64_t* entry_capacity;
    const int64_t* spill_capacity;
    void* record;
};

}  // namespace

struct mld_tracks : mld_batch::Object {
    TrDev d{};
    std::vector<mld_batch::DeviceBuffer<unsigned char>> allocs;  // what the pointers of `d` and the two masks point into
    uint8_t* own_mask = nullptr;  // [n_seq][M]: the masks of a begin without is_new_out
    uint8_t* zero_mask = nullptr; // [M] zeros: the mask the depth call gets for a sequence without a previous frame
    mld_batch::DescRing<TrSeq> ring;
    // host-side frame state: everything a call needs is known when it is issued, nothing is read back
    int committed = 0;      // the table / per-track arrays of the last committed frame
    bool begun = false;
    uint32_t epoch = 0;
    std::vector<int32_t> n_committed, n_pending;
    std::vector<const int32_t*> ids_pending;
    std::vector<uint8_t*> mask_pending;
    std::vector<const uint8_t*> mask_table;  // mld_tracklets_step_device
    std::vector<uint8_t> lane_last;          // mld_tracklets_step_lanes_device: have_last of the lanes that do not restart
    // mld_tracks_set_leaving_sink: copies of the caller's tables, `sink` points at them; consumed by the next step
    bool sink_armed = false;
    LeaveOut sink{};
    std::vector<int32_t*> sink_ids, sink_spill_ids;
    std::vector<int64_t*> sink_offsets;
    std::vector<float*> sink_fp, sink_spill_fp;
    std::vector<int64_t> sink_caps;          // [3][n_seq]: tracks, entries, spills
    std::vector<uint8_t> leave_mode;         // the step's two passes over the sink
};

namespace {

// Block prefixes of the staged descriptors: per sequence ceil(n * per_track / kBlock) blocks, and for the release pass
// ceil(n_prev / kBlock) but at least one.  Returns the two totals.
int layout_blocks(mld_tracks* tr, int per_track, int64_t* total, int64_t* total_prev) {
    int64_t b = 0, bp = 0;
    for (TrSeq& q : tr->ring.stage) {
        q.blk0 = (int32_t)b;
        q.blk0_prev = (int32_t)bp;
        b += ((int64_t)q.n * per_track + kBlock - 1) / kBlock;
        bp += std::max<int64_t>(1, ((int64_t)q.n_prev + kBlock - 1) / kBlock);
        if (b > 0x7fffffff || bp > 0x7fffffff) return fail(tr, MLD_ERR_CAPACITY, "more than 2^31 blocks in one launch");
    }
    *total = b;
    *total_prev = bp;
    return MLD_OK;
}

// What mld_tracks_begin_device refuses, without a change of state.
int check_begin(mld_tracks* tr, const char* fn, const int32_t* const* ids, const int64_t* n_tracks, uint8_t* const* is_new_out) {
    auto refuse = [&](int code, const char* what) {
        tr->err = std::string(fn) + ": " + what;
        return code;
    };
    if (!ids || !n_tracks) return refuse(MLD_ERR_INVALID_ARG, "null table");
    for (int s = 0; s < tr->d.n_seq; s++) {
        if (n_tracks[s] < 0) return refuse(MLD_ERR_INVALID_ARG, "negative track count");
        if (n_tracks[s] > tr->d.M) return refuse(MLD_ERR_CAPACITY, "more tracks than max_tracks");
        if (n_tracks[s] > 0 && (!ids[s] || (is_new_out && !is_new_out[s]))) return refuse(MLD_ERR_INVALID_ARG, "null array");
    }
    return MLD_OK;
}

// What mld_tracks_export_leaving_device refuses, without a change of state.  every_sequence: an array may be null only
// where its capacity is 0 (the sink: the track counts of the step that consumes it are not known yet); otherwise also
// where the sequence has no committed track.
int check_leaving(mld_tracks* tr, const char* fn, const LeaveOut& o, bool every_sequence) {
    auto refuse = [&](const std::string& what) {
        tr->err = std::string(fn) + ": " + what;
        return MLD_ERR_INVALID_ARG;
    };
    if (!o.ids_out) return refuse("null ids_out table");
    if (!o.offsets_out) return refuse("null offsets_out table");
    if (!o.fp_out) return refuse("null fp_out table");
    if (!o.spill_ids_out) return refuse("null spill_ids_out table");
    if (!o.spill_fp_out) return refuse("null spill_fp_out table");
    if (!o.track_capacity) return refuse("null track_capacity");
    if (!o.entry_capacity) return refuse("null entry_capacity");
    if (!o.spill_capacity) return refuse("null spill_capacity");
    if (!o.record) return refuse("null record_out_dev");
    if (mld_batch::misaligned(o.record, 7)) return refuse("record_out_dev is not 8-byte aligned");
    for (int s = 0; s < tr->d.n_seq; s++) {
        if (o.track_capacity[s] < 0) return refuse("negative track_capacity");
        if (o.entry_capacity[s] < 0) return refuse("negative entry_capacity");
        if (o.spill_capacity[s] < 0) return refuse("negative spill_capacity");
        const bool has = every_sequence || tr->n_committed[(size_t)s] > 0;
        if (has && o.track_capacity[s] > 0 && !o.ids_out[s]) return refuse("null ids_out array");
        if (has && o.track_capacity[s] > 0 && !o.offsets_out[s]) return refuse("null offsets_out array");
        if (has && o.entry_capacity[s] > 0 && !o.fp_out[s]) return refuse("null fp_out array");
        if (has && o.spill_capacity[s] > 0 && !o.spill_ids_out[s]) return refuse("null spill_ids_out array");
        if (has && o.spill_capacity[s] > 0 && !o.spill_fp_out[s]) return refuse("null spill_fp_out array");
        if (mld_batch::misaligned(o.ids_out[s], 3)) return refuse("ids_out array is not 4-byte aligned");
        if (mld_batch::misaligned(o.offsets_out[s], 7)) return refuse("offsets_out array is not 8-byte aligned");
        if (mld_batch::misaligned(o.fp_out[s], 3)) return refuse("fp_out array is not 4-byte aligned");
        if (mld_batch::misaligned(o.spill_ids_out[s], 3)) return refuse("spill_ids_out array is not 4-byte aligned");
        if (mld_batch::misaligned(o.spill_fp_out[s], 3)) return refuse("spill_fp_out array is not 4-byte aligned");
    }
    return MLD_OK;
}

// The three launches of the leaving export behind the descriptor upload; mode[s] = kLeaveSkip / kLeaveMarks /
// kLeaveFlush.  `o` has passed check_leaving.  A null array counts as capacity 0.
int queue_leaving(mld_tracks* tr, const LeaveOut& o, const uint8_t* mode) {
    const int S = tr->d.n_seq;
    MLD_HIP(tr, hipSetDevice(tr->device));
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.leave_mode = mode[s];
        if (mode[s] == kLeaveSkip) continue;
        q.ids_out = o.ids_out[s];
        q.offsets_out = o.offsets_out[s];
        q.fp_out = o.fp_out[s];
        q.spill_ids_out = o.spill_ids_out[s];
        q.spill_fp_out = o.spill_fp_out[s];
        q.track_capacity = q.ids_out && q.offsets_out ? o.track_capacity[s] : 0;
        q.capacity = q.fp_out ? o.entry_capacity[s] : 0;
        q.spill_capacity = q.spill_ids_out && q.spill_fp_out ? o.spill_capacity[s] : 0;
        q.n = tr->n_committed[(size_t)s];
    }
    // (layout_blocks reads n_prev, which is leave_mode here: only its second total, which is not used, depends on it)
    int64_t blocks = 0, blocks_prev = 0;
    int rc = layout_blocks(tr, 1, &blocks, &blocks_prev);
    if (rc) return rc;
    if ((rc = tr->ring.upload(tr))) return rc;
    if (blocks > 0) {
        hipLaunchKernelGGL(k_tracks_leave_sums, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(),
                           tr->committed, tr->epoch);
        MLD_HIP(tr, hipGetLastError());
    }
    hipLaunchKernelGGL(k_tracks_leave_scan, dim3((unsigned)S), dim3(kScanWidth), 0, tr->stream, tr->d, tr->ring.d_desc.get(),
                       static_cast<long long*>(o.record));
    MLD_HIP(tr, hipGetLastError());
    if (blocks > 0) {
        hipLaunchKernelGGL(k_tracks_leave_write, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(),
                           tr->committed);
        MLD_HIP(tr, hipGetLastError());
    }
    return MLD_OK;
}

template <typename T>
int dev_alloc(mld_tracks* tr, T** p, size_t count, bool zero) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 4);
    tr->allocs.emplace_back();
    const int rc = tr->allocs.back().allocate(tr, bytes);
    if (rc) return rc;
    void* q = tr->allocs.back().get();
    if (zero) MLD_HIP(tr, hipMemsetAsync(q, 0, bytes, tr->stream));
    *p = static_cast<T*>(q);
    return MLD_OK;
}

int allocate(mld_tracks* tr) {
    TrDev& d = tr->d;
    const size_t S = (size_t)d.n_seq, M = (size_t)d.M, H = (size_t)d.H;
    int rc;
    if ((rc = dev_alloc(tr, &d.table, 2 * S * d.cap, true))) return rc;
    if ((rc = dev_alloc(tr, &d.hist, S * M * H * 3, false))) return rc;
    if ((rc = dev_alloc(tr, &d.head, S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &d.len, S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &d.mark, S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &d.free_rows, S * M, false))) return rc;
    if ((rc = dev_alloc(tr, &d.top, S, false))) return rc;
    if ((rc = dev_alloc(tr, &d.row, 2 * S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &d.slot, 2 * S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &d.dup_row, 2 * S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &d.cnt, S * 4, true))) return rc;
    if ((rc = dev_alloc(tr, &d.feat, S * 2, true))) return rc;
    const size_t pack_blocks = S * ((M + kBlock - 1) / kBlock);
    if ((rc = dev_alloc(tr, &d.pack_sum, pack_blocks, false))) return rc;
    if ((rc = dev_alloc(tr, &d.pack_base, pack_blocks, false))) return rc;
    if ((rc = dev_alloc(tr, &d.pack_meta, S * M, false))) return rc;
    if ((rc = dev_alloc(tr, &tr->own_mask, S * M, true))) return rc;
    if ((rc = dev_alloc(tr, &tr->zero_mask, M, true))) return rc;
    if ((rc = tr->ring.allocate(tr, d.n_seq))) return rc;
    // (the table starts as zeros, like the rest of the store's memory)
    MLD_HIP(tr, hipMemsetAsync(tr->ring.d_desc.get(), 0, tr->ring.gen_bytes, tr->stream));
    const size_t total = std::max(S * M, S);
    hipLaunchKernelGGL(k_tracks_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, tr->stream, d);
    MLD_HIP(tr, hipGetLastError());
    return MLD_OK;
}

}  // namespace

extern "C" {

mld_tracks* mld_tracks_create(mld_ctx* ctx, int n_seq, int64_t max_tracks, int max_history, int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_tracks_create: n_seq must be in 1 .. 65536";
        if (max_tracks < 1 || max_tracks > (1 << 24)) return "mld_tracks_create: max_tracks must be in 1 .. 16777216";
        if (max_history < 2 || max_history > 65535) return "mld_tracks_create: max_history must be in 2 .. 65535";
        if (!ctx) return "mld_tracks_create: null context";
        return nullptr;
    };
    auto init = [&](mld_tracks* tr) {
        tr->d.n_seq = n_seq;
        tr->d.M = (int32_t)max_tracks;
        tr->d.H = max_history;
        uint32_t cap = 2;
        while (cap < 2u * (uint32_t)max_tracks) cap <<= 1;
        tr->d.cap = cap;
        tr->n_committed.assign((size_t)n_seq, 0);
        tr->n_pending.assign((size_t)n_seq, 0);
        tr->ids_pending.assign((size_t)n_seq, nullptr);
        tr->mask_pending.assign((size_t)n_seq, nullptr);
        tr->mask_table.assign((size_t)n_seq, nullptr);
        tr->lane_last.assign((size_t)n_seq, 0);
        tr->leave_mode.assign((size_t)n_seq, 0);
        return allocate(tr);
    };
    return mld_batch::create_object<mld_tracks>(g_create_error, "mld_tracks_create", refusal(), ctx, status_out, init);
}

void mld_tracks_destroy(mld_tracks* tr) { mld_batch::destroy_object(tr); }

const char* mld_tracks_last_error(const mld_tracks* tr) { return tr ? tr->err.c_str() : g_create_error; }

int mld_tracks_begin_device(mld_tracks* tr, const int32_t* const* ids, const int64_t* n_tracks, uint8_t* const* is_new_out) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    int rc = check_begin(tr, "mld_tracks_begin_device", ids, n_tracks, is_new_out);
    if (rc) return rc;
    const int S = tr->d.n_seq;
    MLD_HIP(tr, hipSetDevice(tr->device));
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.ids = ids[s];
        q.is_new = is_new_out ? is_new_out[s] : tr->own_mask + (size_t)s * tr->d.M;
        q.n = (int32_t)n_tracks[s];
        q.n_prev = tr->n_committed[(size_t)s];
        tr->n_pending[(size_t)s] = q.n;
        tr->ids_pending[(size_t)s] = q.ids;
        tr->mask_pending[(size_t)s] = q.is_new;
    }
    // a frame begun twice: the later look-up stamps a new epoch, the marks of the abandoned one mean nothing
    tr->epoch++;
    tr->begun = true;
    int64_t blocks = 0, blocks_prev = 0;
    if ((rc = layout_blocks(tr, 1, &blocks, &blocks_prev))) return rc;
    if (blocks == 0) return MLD_OK;
    if ((rc = tr->ring.upload(tr))) return rc;
    hipLaunchKernelGGL(k_tracks_lookup, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed,
                       tr->epoch);
    MLD_HIP(tr, hipGetLastError());
    return MLD_OK;
}

int mld_tracks_commit_device(mld_tracks* tr, const float* const* u_new, const float* const* v_new, const float* const* u_old,
                             const float* const* v_old, const float* const* d_cur, const float* const* d_last) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!tr->begun) return fail(tr, MLD_ERR_NOT_INITIALIZED, "mld_tracks_commit_device without mld_tracks_begin_device");
    if (!u_new || !v_new || !u_old || !v_old || !d_cur || !d_last)
        return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_commit_device: null table");
    const int S = tr->d.n_seq;
    for (int s = 0; s < S; s++)
        if (tr->n_pending[(size_t)s] > 0 && (!u_new[s] || !v_new[s] || !u_old[s] || !v_old[s] || !d_cur[s] || !d_last[s]))
            return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_commit_device: null array");
    MLD_HIP(tr, hipSetDevice(tr->device));
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.ids = tr->ids_pending[(size_t)s];
        q.is_new = tr->mask_pending[(size_t)s];
        q.u_new = u_new[s];
        q.v_new = v_new[s];
        q.u_old = u_old[s];
        q.v_old = v_old[s];
        q.d_cur = d_cur[s];
        q.d_last = d_last[s];
        q.n = tr->n_pending[(size_t)s];
        q.n_prev = tr->n_committed[(size_t)s];
    }
    int64_t blocks = 0, blocks_prev = 0;
    int rc = layout_blocks(tr, 1, &blocks, &blocks_prev);
    if (rc) return rc;
    if ((rc = tr->ring.upload(tr))) return rc;
    hipLaunchKernelGGL(k_tracks_release, dim3((unsigned)blocks_prev), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(),
                       tr->committed, tr->epoch);
    MLD_HIP(tr, hipGetLastError());
    if (blocks > 0) {
        hipLaunchKernelGGL(k_tracks_commit, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(),
                           1 - tr->committed);
        MLD_HIP(tr, hipGetLastError());
    }
    tr->committed = 1 - tr->committed;
    tr->n_committed = tr->n_pending;
    tr->begun = false;
    return MLD_OK;
}

int mld_tracks_export_device(mld_tracks* tr, float* const* fp_out, int32_t* const* len_out) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!fp_out && !len_out) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_device: nothing to write");
    const int S = tr->d.n_seq;
    for (int s = 0; s < S; s++)
        if (tr->n_committed[(size_t)s] > 0 && ((fp_out && !fp_out[s]) || (len_out && !len_out[s])))
            return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_device: null array");
    MLD_HIP(tr, hipSetDevice(tr->device));
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.fp_out = fp_out ? fp_out[s] : nullptr;
        q.len_out = len_out ? len_out[s] : nullptr;
        q.n = tr->n_committed[(size_t)s];
    }
    int64_t blocks = 0, blocks_prev = 0;
    int rc = layout_blocks(tr, tr->d.H, &blocks, &blocks_prev);
    if (rc) return rc;
    if (blocks == 0) return MLD_OK;
    if ((rc = tr->ring.upload(tr))) return rc;
    hipLaunchKernelGGL(k_tracks_export, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed);
    MLD_HIP(tr, hipGetLastError());
    return MLD_OK;
}

int mld_tracks_export_packed_device(mld_tracks* tr, float* const* fp_out, const int64_t* capacity,
                                    int64_t* const* offsets_out) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!offsets_out) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_packed_device: null offsets_out table");
    if (fp_out && !capacity) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_packed_device: fp_out without capacity");
    const int S = tr->d.n_seq;
    for (int s = 0; s < S; s++) {
        if (fp_out && capacity[s] < 0) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_packed_device: negative capacity");
        if (tr->n_committed[(size_t)s] > 0 && !offsets_out[s])
            return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_packed_device: null offsets_out array");
        if (tr->n_committed[(size_t)s] > 0 && fp_out && !fp_out[s] && capacity[s] > 0)  // (no entries need no array)
            return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_export_packed_device: null fp_out array");
    }
    MLD_HIP(tr, hipSetDevice(tr->device));
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.fp_out = fp_out ? fp_out[s] : nullptr;
        q.capacity = q.fp_out ? capacity[s] : 0;
        q.offsets_out = offsets_out[s];
        q.n = tr->n_committed[(size_t)s];
    }
    int64_t blocks = 0, blocks_prev = 0;
    int rc = layout_blocks(tr, 1, &blocks, &blocks_prev);
    if (rc) return rc;
    if (blocks == 0) return MLD_OK;
    if ((rc = tr->ring.upload(tr))) return rc;
    hipLaunchKernelGGL(k_tracks_pack_sums, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed);
    MLD_HIP(tr, hipGetLastError());
    hipLaunchKernelGGL(k_tracks_pack_scan, dim3((unsigned)S), dim3(kScanWidth), 0, tr->stream, tr->d, tr->ring.d_desc.get());
    MLD_HIP(tr, hipGetLastError());
    hipLaunchKernelGGL(k_tracks_pack_write, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed);
    MLD_HIP(tr, hipGetLastError());
    return MLD_OK;
}

int mld_tracks_export_leaving_device(mld_tracks* tr, const uint8_t* flush, int32_t* const* ids_out, int64_t* const* offsets_out,
                                     float* const* fp_out, int32_t* const* spill_ids_out, float* const* spill_fp_out,
                                     const int64_t* track_capacity, const int64_t* entry_capacity, const int64_t* spill_capacity,
                                     void* record_out_dev) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    const LeaveOut o{ids_out, offsets_out, fp_out, spill_ids_out, spill_fp_out, track_capacity, entry_capacity, spill_capacity,
                     record_out_dev};
    int rc = check_leaving(tr, "mld_tracks_export_leaving_device", o, false);
    if (rc) return rc;
    const int S = tr->d.n_seq;
    bool all_flushed = flush != nullptr;
    for (int s = 0; s < S; s++) {
        tr->leave_mode[(size_t)s] = flush && flush[s] ? kLeaveFlush : kLeaveMarks;
        all_flushed = all_flushed && flush[s] != 0;
    }
    if (!tr->begun && !all_flushed)
        return fail(tr, MLD_ERR_NOT_INITIALIZED,
                    "mld_tracks_export_leaving_device without mld_tracks_begin_device (only a flush of every sequence needs none)");
    return queue_leaving(tr, o, tr->leave_mode.data());
}

int mld_tracks_set_leaving_sink(mld_tracks* tr, int32_t* const* ids_out, int64_t* const* offsets_out, float* const* fp_out,
                                int32_t* const* spill_ids_out, float* const* spill_fp_out, const int64_t* track_capacity,
                                const int64_t* entry_capacity, const int64_t* spill_capacity, void* record_out_dev) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!ids_out && !offsets_out && !fp_out && !spill_ids_out && !spill_fp_out && !track_capacity && !entry_capacity &&
        !spill_capacity && !record_out_dev) {  // (all null: the sink is taken away)
        tr->sink_armed = false;
        return MLD_OK;
    }
    const LeaveOut o{ids_out, offsets_out, fp_out, spill_ids_out, spill_fp_out, track_capacity, entry_capacity, spill_capacity,
                     record_out_dev};
    const int rc = check_leaving(tr, "mld_tracks_set_leaving_sink", o, true);
    if (rc) return rc;  // (a sink armed before stays as it was)
    const size_t S = (size_t)tr->d.n_seq;
    tr->sink_ids.assign(ids_out, ids_out + S);
    tr->sink_offsets.assign(offsets_out, offsets_out + S);
    tr->sink_fp.assign(fp_out, fp_out + S);
    tr->sink_spill_ids.assign(spill_ids_out, spill_ids_out + S);
    tr->sink_spill_fp.assign(spill_fp_out, spill_fp_out + S);
    tr->sink_caps.assign(track_capacity, track_capacity + S);
    tr->sink_caps.insert(tr->sink_caps.end(), entry_capacity, entry_capacity + S);
    tr->sink_caps.insert(tr->sink_caps.end(), spill_capacity, spill_capacity + S);
    tr->sink = LeaveOut{tr->sink_ids.data(), tr->sink_offsets.data(), tr->sink_fp.data(), tr->sink_spill_ids.data(),
                        tr->sink_spill_fp.data(), tr->sink_caps.data(), tr->sink_caps.data() + S, tr->sink_caps.data() + 2 * S,
                        record_out_dev};
    tr->sink_armed = true;
    return MLD_OK;
}

}  // extern "C"

namespace {

// The selected sequences emptied and, with tables, loaded: mld_tracks_import_packed_device, mld_tracks_reset_device
// (ids == nullptr: no tracks anywhere) and the restart of mld_tracklets_step_lanes_device.  Everything is checked before
// anything is queued or any host state changes.
int import_packed(mld_tracks* tr, const char* fn, const uint8_t* select, const int32_t* const* ids, const int64_t* n_tracks,
                  const int64_t* const* offsets, const float* const* fp, const int64_t* n_entries) {
    auto refuse = [&](int code, const char* what) {
        tr->err = std::string(fn) + ": " + what;
        return code;
    };
    const int S = tr->d.n_seq;
    const bool load = ids != nullptr;
    if (load && (!n_tracks || !offsets || !fp || !n_entries)) return refuse(MLD_ERR_INVALID_ARG, "null table");
    const int64_t reset_blocks = ((int64_t)tr->d.cap + kBlock - 1) / kBlock;
    int64_t blocks = 0, blocks_reset = 0;
    for (int s = 0; s < S; s++) {
        if (select && !select[s]) continue;
        blocks_reset += reset_blocks;
        if (!load) continue;
        if (n_tracks[s] < 0) return refuse(MLD_ERR_INVALID_ARG, "negative track count");
        if (n_entries[s] < 0) return refuse(MLD_ERR_INVALID_ARG, "negative n_entries");
        if (n_tracks[s] > tr->d.M) return refuse(MLD_ERR_CAPACITY, "more tracks than max_tracks");
        // (without entries nothing of fp[s] is read: every track is stored with length 0)
        if (n_tracks[s] > 0 && (!ids[s] || !offsets[s] || (!fp[s] && n_entries[s] > 0)))
            return refuse(MLD_ERR_INVALID_ARG, "null array");
        blocks += (n_tracks[s] + kBlock - 1) / kBlock;
    }
    if (blocks > 0x7fffffff || blocks_reset > 0x7fffffff) return refuse(MLD_ERR_CAPACITY, "more than 2^31 blocks in one launch");
    MLD_HIP(tr, hipSetDevice(tr->device));
    int64_t b = 0, br = 0;
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.blk0 = (int32_t)b;
        q.blk0_prev = (int32_t)br;
        if (select && !select[s]) continue;  // (no block of either launch: the sequence is not touched)
        br += reset_blocks;
        if (load && n_tracks[s] > 0) {
            q.ids = ids[s];
            q.offsets_in = offsets[s];
            q.fp_in = fp[s];
            q.n_entries = n_entries[s];
            q.n = (int32_t)n_tracks[s];
            b += ((int64_t)q.n + kBlock - 1) / kBlock;
        }
    }
    if (blocks_reset > 0) {
        int rc = tr->ring.upload(tr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_tracks_reset, dim3((unsigned)blocks_reset), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed);
        MLD_HIP(tr, hipGetLastError());
        if (blocks > 0) {
            hipLaunchKernelGGL(k_tracks_import, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed);
            MLD_HIP(tr, hipGetLastError());
        }
    }
    // the host's view follows what was queued (as in mld_tracks_commit_device)
    for (int s = 0; s < S; s++)
        if (!select || select[s]) tr->n_committed[(size_t)s] = tr->ring.stage[(size_t)s].n;
    tr->begun = false;  // a begun frame is abandoned: its look-up saw what the import replaces
    return MLD_OK;
}

}  // namespace

extern "C" {

int mld_tracks_import_packed_device(mld_tracks* tr, const uint8_t* select, const int32_t* const* ids, const int64_t* n_tracks,
                                    const int64_t* const* offsets, const float* const* fp, const int64_t* n_entries) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!ids) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_import_packed_device: null table");
    return import_packed(tr, "mld_tracks_import_packed_device", select, ids, n_tracks, offsets, fp, n_entries);
}

int mld_tracks_reset_device(mld_tracks* tr, const uint8_t* select) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    return import_packed(tr, "mld_tracks_reset_device", select, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int mld_tracks_counts(mld_tracks* tr, int64_t* counts_out) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!counts_out) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracks_counts: null output");
    const int S = tr->d.n_seq;
    MLD_HIP(tr, hipSetDevice(tr->device));
    for (int s = 0; s < S; s++) {
        TrSeq& q = tr->ring.stage[(size_t)s];
        q = TrSeq{};
        q.n = tr->n_committed[(size_t)s];
    }
    int64_t blocks = 0, blocks_prev = 0;
    int rc = layout_blocks(tr, 1, &blocks, &blocks_prev);
    if (rc) return rc;
    MLD_HIP(tr, hipMemsetAsync(tr->d.feat, 0, (size_t)S * 2 * sizeof(unsigned long long), tr->stream));
    if (blocks > 0) {
        if ((rc = tr->ring.upload(tr))) return rc;
        hipLaunchKernelGGL(k_tracks_count, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->d, tr->ring.d_desc.get(), tr->committed);
        MLD_HIP(tr, hipGetLastError());
    }
    std::vector<unsigned int> cnt((size_t)S * 4);
    std::vector<unsigned long long> feat((size_t)S * 2);
    MLD_HIP(tr, hipMemcpyAsync(cnt.data(), tr->d.cnt, cnt.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, tr->stream));
    MLD_HIP(tr, hipMemcpyAsync(feat.data(), tr->d.feat, feat.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, tr->stream));
    MLD_HIP(tr, hipStreamSynchronize(tr->stream));
    for (int s = 0; s < S; s++) {
        int64_t* c = counts_out + (size_t)s * 6;
        c[1] = cnt[(size_t)s * 4 + 0];
        c[2] = cnt[(size_t)s * 4 + 1];
        c[0] = c[1] + c[2];
        c[3] = (int64_t)feat[(size_t)s * 2 + 0];
        c[4] = (int64_t)feat[(size_t)s * 2 + 1];
        c[5] = cnt[(size_t)s * 4 + 2];
    }
    return MLD_OK;
}

// mld_tracklets_depths_device with have_last per sequence, on that call alone (the depth path is not touched).  Equal
// flags: that call.  Mixed flags: the sequences with a previous frame and those without go through it one group after the
// other, each call with the other group's track counts at zero - a sequence without tracks has no feature on either of
// its slots, so nothing of its previous-bank slot is read, and the group without a previous frame is answered -1 /
// MLD_Unspecified.  The call with have_last = 1 checks the previous-bank slot of EVERY sequence as it always does
// (include/mld.h states it).  (The step below needs one launch set only: it owns the masks.)
int mld_tracklets_depths_lanes_device(mld_ctx* ctx, int n_seq, int bank_cur, const uint8_t* have_last, const float* const* u_new,
                                      const float* const* v_new, const float* const* u_old, const float* const* v_old,
                                      const uint8_t* const* is_new, const int64_t* n_tracks, float* const* d_cur_out,
                                      float* const* d_last_out, int32_t* const* type_cur_out, int32_t* const* type_last_out) {
    if (!ctx || !have_last || n_seq < 1) return MLD_ERR_INVALID_ARG;
    int with = 0;
    for (int q = 0; q < n_seq; q++) with += have_last[q] != 0;
    if (with == 0 || with == n_seq || !n_tracks)  // (a null table: the call's own refusal)
        return mld_tracklets_depths_device(ctx, n_seq, bank_cur, with ? 1 : 0, u_new, v_new, u_old, v_old, is_new, n_tracks,
                                           d_cur_out, d_last_out, type_cur_out, type_last_out);
    std::vector<int64_t> n_with((size_t)n_seq), n_without((size_t)n_seq);
    for (int q = 0; q < n_seq; q++) {
        n_with[(size_t)q] = have_last[q] ? n_tracks[q] : 0;
        n_without[(size_t)q] = have_last[q] ? 0 : n_tracks[q];
    }
    const int rc = mld_tracklets_depths_device(ctx, n_seq, bank_cur, 1, u_new, v_new, u_old, v_old, is_new, n_with.data(),
                                               d_cur_out, d_last_out, type_cur_out, type_last_out);
    if (rc) return rc;
    return mld_tracklets_depths_device(ctx, n_seq, bank_cur, 0, u_new, v_new, u_old, v_old, is_new, n_without.data(), d_cur_out,
                                       d_last_out, type_cur_out, type_last_out);
}

// have_last == nullptr: the scalar call (`uniform` for every sequence, no restart).
static int tracklets_step(const char* fn, mld_ctx* ctx, mld_tracks* tr, int bank_cur, int uniform, const uint8_t* have_last,
                          const uint8_t* restart, const int32_t* const* ids, const float* const* u_new,
                          const float* const* v_new, const float* const* u_old, const float* const* v_old,
                          const int64_t* n_tracks, float* const* d_cur_out, float* const* d_last_out,
                          int32_t* const* type_cur_out, int32_t* const* type_last_out) {
    auto refuse = [&](const char* what) {
        tr->err = std::string(fn) + ": " + what;
        return MLD_ERR_INVALID_ARG;
    };
    if (!ctx || ctx != tr->ctx) return refuse("the store belongs to another context");
    if (!d_cur_out || !d_last_out) return refuse("null output table");
    const int S = tr->d.n_seq;
    int rc;
    bool any_restart = false;
    for (int s = 0; restart && s < S; s++) any_restart = any_restart || restart[s] != 0;
    // A sink (mld_tracks_set_leaving_sink) takes what this step removes from the store, every sequence in exactly one
    // of two passes: the restarting ones whole, before they are emptied; the others by the marks of this step's look-up.
    const bool sink = tr->sink_armed;
    if (any_restart || sink) {  // (what the begin would refuse is refused before a lane is emptied or the sink written)
        if ((rc = check_begin(tr, fn, ids, n_tracks, nullptr))) return rc;
    }
    if (any_restart) {
        if (sink) {
            for (int s = 0; s < S; s++) tr->leave_mode[(size_t)s] = restart[s] ? kLeaveFlush : kLeaveSkip;
            if ((rc = queue_leaving(tr, tr->sink, tr->leave_mode.data()))) return rc;
        }
        if ((rc = import_packed(tr, fn, restart, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
    }
    if ((rc = mld_tracks_begin_device(tr, ids, n_tracks, nullptr))) return rc;
    if (sink) {
        for (int s = 0; s < S; s++) tr->leave_mode[(size_t)s] = any_restart && restart[s] ? kLeaveSkip : kLeaveMarks;
        tr->sink_armed = false;  // one step, whatever becomes of it from here on
        if ((rc = queue_leaving(tr, tr->sink, tr->leave_mode.data()))) return rc;
    }
    for (int s = 0; s < S; s++) tr->mask_table[(size_t)s] = tr->mask_pending[(size_t)s];
    int with = 0;
    for (int s = 0; have_last && s < S; s++) {
        tr->lane_last[(size_t)s] = have_last[s] && !(restart && restart[s]) ? 1 : 0;
        with += tr->lane_last[(size_t)s];
    }
    const bool mixed = have_last && with > 0 && with < S;
    if (have_last && !mixed) uniform = with > 0;
    // Mixed flags, ONE launch set: the depth call runs with have_last = 1 and sees an all-zero mask for a sequence
    // without a previous frame - no previous feature of it is evaluated, nothing of its previous-bank slot is read and
    // its d_last is not written; k_tracks_no_previous then answers its new tracks as the call without a cloud would.
    if (mixed)
        for (int s = 0; s < S; s++)
            if (!tr->lane_last[(size_t)s]) tr->mask_table[(size_t)s] = tr->zero_mask;
    rc = mld_tracklets_depths_device(ctx, S, bank_cur, mixed ? 1 : uniform, u_new, v_new, u_old, v_old, tr->mask_table.data(),
                                     n_tracks, d_cur_out, d_last_out, type_cur_out, type_last_out);
    if (rc) {  // (the frame stays begun and uncommitted: the next begin replaces it)
        tr->err = std::string("mld_tracklets_depths_device: ") + mld_last_error(ctx);
        return rc;
    }
    if (mixed) {
        for (int s = 0; s < S; s++) {
            TrSeq& q = tr->ring.stage[(size_t)s];
            q = TrSeq{};
            if (tr->lane_last[(size_t)s]) continue;  // (no block: layout_blocks gives blocks to n > 0 only)
            q.is_new = tr->mask_pending[(size_t)s];
            q.d_last_w = d_last_out[s];
            q.len_out = type_last_out ? type_last_out[s] : nullptr;
            q.n = tr->n_pending[(size_t)s];
        }
        int64_t blocks = 0, blocks_prev = 0;
        if ((rc = layout_blocks(tr, 1, &blocks, &blocks_prev))) return rc;
        if (blocks > 0) {
            if ((rc = tr->ring.upload(tr))) return rc;
            hipLaunchKernelGGL(k_tracks_no_previous, dim3((unsigned)blocks), dim3(kBlock), 0, tr->stream, tr->ring.d_desc.get(), S);
            MLD_HIP(tr, hipGetLastError());
        }
    }
    return mld_tracks_commit_device(tr, u_new, v_new, u_old, v_old, d_cur_out, d_last_out);
}

int mld_tracklets_step_device(mld_ctx* ctx, mld_tracks* tr, int bank_cur, int have_last, const int32_t* const* ids,
                              const float* const* u_new, const float* const* v_new, const float* const* u_old,
                              const float* const* v_old, const int64_t* n_tracks, float* const* d_cur_out,
                              float* const* d_last_out, int32_t* const* type_cur_out, int32_t* const* type_last_out) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    return tracklets_step("mld_tracklets_step_device", ctx, tr, bank_cur, have_last, nullptr, nullptr, ids, u_new, v_new, u_old,
                          v_old, n_tracks, d_cur_out, d_last_out, type_cur_out, type_last_out);
}

int mld_tracklets_step_lanes_device(mld_ctx* ctx, mld_tracks* tr, int bank_cur, const uint8_t* have_last, const uint8_t* restart,
                                    const int32_t* const* ids, const float* const* u_new, const float* const* v_new,
                                    const float* const* u_old, const float* const* v_old, const int64_t* n_tracks,
                                    float* const* d_cur_out, float* const* d_last_out, int32_t* const* type_cur_out,
                                    int32_t* const* type_last_out) {
    if (!tr) return MLD_ERR_INVALID_ARG;
    if (!have_last) return fail(tr, MLD_ERR_INVALID_ARG, "mld_tracklets_step_lanes_device: null have_last");
    return tracklets_step("mld_tracklets_step_lanes_device", ctx, tr, bank_cur, 0, have_last, restart, ids, u_new, v_new, u_old,
                          v_old, n_tracks, d_cur_out, d_last_out, type_cur_out, type_last_out);
}

}  // extern "C"
