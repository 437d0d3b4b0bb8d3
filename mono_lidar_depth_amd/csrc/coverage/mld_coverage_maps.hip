// mld_coverage_maps.hip — where in the image a feature can get a depth, for a batch of sequences in one call (include/mld.h,
// "mld_coverage_maps"): the neighbour stage of the per-feature path - the window rule of NeighborFinderPixel::getNeighbors
// (NeighborFinderPixel.cpp:60-95), the count test (DepthEstimator.cpp:680-681) and what decides whether the road fallback
// can run (:585-586, :782-830) - evaluated at EVERY integer pixel of every sequence.  The inputs are the arrays
// mld_projected_clouds_export_device writes (pixel map, _pointIndex, camera-frame cloud) and, optionally, the plane
// mld_semantic_planes / mld_ransac_planes leave on the device.  Everything here is an exact integer; no frame slot is
// involved, nothing is allocated per call and nothing comes back to the host.
//
// Four launches: the descriptor upload and
//   k_coverage_classify  one wavefront per 64 cells of a map row: occupied / inlier / far as three ballots = one 64-bit word
//                        of each of three bit planes (a row: ceil(W / 64) words); cell counts and the bad-input flag as
//                        block partials.  The map and the index are read here and nowhere else.
//   k_coverage_count     one block per tile of 256 columns x BR rows, a thread per column: the column bounds in registers,
//                        the row bounds of the band in LDS, both by the f64 rule; the tile's words of the bit planes (band +
//                        halo, at most six words a row) staged in LDS in one coalesced pass; per row of the tile the
//                        horizontal part of the four counts as popcounts of one or two masked words, summed down the
//                        column into a prefix held in LDS (4 x 16 bits in one 64-bit entry); a pixel's counts are then two
//                        differences of prefix entries.  Writes the maps, reach, the unsaturated narrow count for the
//                        buckets, and pixel counts as block partials.
//   k_coverage_finish    per sequence: the record from the block partials of both kernels; one wavefront per bucket.  (The
//                        record is summed here and not in k_coverage_count: there it would need a hand-off between blocks.)
// The only ordering between blocks is the boundary between two launches: no atomics, no flags, no fences.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, the wavefront helpers and the size
// limits: ../batch/mld_batch_device.h).  The window rule, the far test and the mask bit are those of k_feature_trace, the
// one copy in ../batch/mld_depth_path.h; Tinv and the half sizes are formed by that header as mld_create forms them, and the
// refusals mld_create shares with this object are its functions.  This unit is compiled without contraction like the rest
// of the library.
#include <hip/hip_runtime.h>

#include <cmath>
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

constexpr int kBlock = 256;           // threads of every kernel here = columns of a tile
constexpr int kWaves = kBlock / kWave;
constexpr int kWordsPerWave = 4;      // k_coverage_classify: words of the bit planes a wavefront makes
constexpr int kWordsPerBlock = kWaves * kWordsPerWave;
constexpr int kMaxSpan = 64;          // columns / rows the wide window may span: a row's part lies in at most two words
constexpr int kMaxBand = 16;          // rows of a band (BR)
constexpr int kStageWords = 6;        // words of a bit-plane row a tile's windows reach: 256 columns and up to 63 either side
constexpr int64_t kMaxGrid = 2147483647;

static_assert(sizeof(mld_coverage_record) == 64, "64 bytes per record (include/mld.h)");
static_assert(offsetof(mld_coverage_record, n_occupied) == 16 && offsetof(mld_coverage_record, max_nb) == 40 &&
                  offsetof(mld_coverage_record, n_buckets) == 48,
              "field offsets of the record (include/mld.h)");

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct CvSeq {
    const int32_t* map;    // W * H: visible index or -1
    const int32_t* index;  // index_len: original index of a visible point
    const double* cam;     // 3 x n_points
    const uint32_t* mask;  // ceil(n_points / 32) words; read only with has_plane
    uint8_t* nb;           // the five maps, W * H each, or null
    uint8_t* road;
    uint8_t* road_inl;
    uint8_t* road_far;
    uint8_t* reach;
    int32_t* bucket;       // 3 x bucket_cap, or null
    float coeffs[4];
    int32_t index_len;
    int32_t n_points;
    int32_t bucket_cap;
    int32_t has_plane;
};
static_assert(sizeof(CvSeq) == 112, "112 bytes per sequence (include/mld.h, DESIGN.md)");

struct CvCalib {
    double Tinv[12];  // camera -> lidar (DepthEstimator.cpp:44)
    double halfX1, halfY1, halfX2, halfY2;
    double roadDistThr;
    int32_t W, H, WW;   // WW: 64-bit words of a bit-plane row
    uint32_t countMin;
    int32_t allZero;    // set_all_depths_to_zero: no feature takes the path (DepthEstimator.cpp:448-453)
    int32_t BR;         // rows of a band
    int32_t tileRows;   // prefix rows a tile may need (its rows + the zero row in front)
    int32_t blocksA;    // blocks of k_coverage_classify per sequence
    int32_t strips, bands;  // tiles of k_coverage_count per sequence: strips * bands
};

// What a call asks of k_coverage_count and k_coverage_finish besides the descriptors.
struct CvCall {
    mld_coverage_record* record;  // n_seq records
    int32_t bucket_w, bucket_h;   // 0: the call has no buckets
    int32_t nbx, nby;             // buckets across and down
};

// The words and masks of the columns lo .. hi (at most 64 of them) in a bit-plane row.
struct ColSpan {
    int w0, w1;
    unsigned long long m0, m1;
};
__device__ __forceinline__ ColSpan col_span(int lo, int hi) {
    ColSpan s;
    s.w0 = lo >> 6;
    s.w1 = hi >> 6;
    const unsigned long long from = ~0ull << (lo & 63), upto = ~0ull >> (63 - (hi & 63));
    if (s.w0 == s.w1) {
        s.m0 = from & upto;
        s.m1 = 0ull;
    } else {
        s.m0 = from;
        s.m1 = upto;
    }
    return s;
}
__device__ __forceinline__ int span_count(const unsigned long long* row, const ColSpan& s) {
    return (int)__popcll(row[s.w0] & s.m0) + (int)__popcll(row[s.w1] & s.m1);
}

__device__ __forceinline__ MLD_BATCH_GLOBAL unsigned long long* plane_row(unsigned long long* planes, const CvCalib& c, int s, int p,
                                                                         int y) {
    return as_global(planes) + ((size_t)(3 * s + p) * (size_t)c.H + (size_t)y) * (size_t)c.WW;
}

// Grid: n_seq * blocksA blocks; a wavefront makes kWordsPerWave consecutive words of the planes (row-major over the rows'
// words).  partA: per block (occupied, inlier, far, bad input).
__global__ __launch_bounds__(kBlock) void k_coverage_classify(const CvSeq* __restrict__ desc, CvCalib c, unsigned long long* planes,
                                                              int32_t* partA) {
    __shared__ int wsum[kWaves][4];
    const int s = (int)(blockIdx.x / (unsigned)c.blocksA), blk = (int)(blockIdx.x % (unsigned)c.blocksA);
    const CvSeq q = desc[s];
    const int lane = (int)threadIdx.x & (kWave - 1), w = (int)threadIdx.x >> 6;
    const long long nwords = (long long)c.WW * (long long)c.H;
    const MLD_BATCH_GLOBAL int32_t* map = as_global(q.map);
    const MLD_BATCH_GLOBAL int32_t* index = as_global(q.index);
    const MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    const MLD_BATCH_GLOBAL uint32_t* mask = as_global(q.mask);
    int n_occ = 0, n_inl = 0, n_far = 0;
    bool badl = false;
    // The loads of the wavefront's words in stages - every map value, then every index, then every point and mask word -
    // so that a wavefront waits for three loads in a row and not for three per word.
    const long long w0 = (long long)blk * kWordsPerBlock + (long long)(w * kWordsPerWave);  // (uniform in the wavefront)
    int ys[kWordsPerWave], wxs[kWordsPerWave], m[kWordsPerWave], orig[kWordsPerWave];
    bool has[kWordsPerWave];
#pragma unroll
    for (int k = 0; k < kWordsPerWave; k++) {
        const long long wi = w0 + k;
        ys[k] = (int)(wi / c.WW);
        wxs[k] = (int)(wi - (long long)ys[k] * c.WW);
        const int x = wxs[k] * kWave + lane;
        m[k] = (wi < nwords && x < c.W) ? map[(size_t)x + (size_t)ys[k] * (size_t)c.W] : -1;
    }
#pragma unroll
    for (int k = 0; k < kWordsPerWave; k++) {
        const bool in_index = m[k] >= 0 && m[k] < q.index_len;
        if (m[k] != -1 && !in_index) badl = true;
        orig[k] = in_index ? index[m[k]] : -1;
    }
#pragma unroll
    for (int k = 0; k < kWordsPerWave; k++) {
        const bool in_index = m[k] >= 0 && m[k] < q.index_len;
        has[k] = in_index && orig[k] >= 0 && orig[k] < q.n_points;
        if (in_index && !has[k]) badl = true;
    }
    double px[kWordsPerWave], py[kWordsPerWave], pz[kWordsPerWave];
    uint32_t mw[kWordsPerWave];
    if (q.has_plane) {
#pragma unroll
        for (int k = 0; k < kWordsPerWave; k++) {
            px[k] = py[k] = pz[k] = 0.0;
            mw[k] = 0u;
            if (has[k]) {
                px[k] = cam[3 * (size_t)orig[k]], py[k] = cam[3 * (size_t)orig[k] + 1], pz[k] = cam[3 * (size_t)orig[k] + 2];
                mw[k] = mask[(unsigned)orig[k] >> 5];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kWordsPerWave; k++) {
        if (w0 + k >= nwords) break;
        const unsigned long long mo = __ballot(has[k]);
        n_occ += (int)__popcll(mo);
        unsigned long long mi = 0ull, mf = 0ull;
        if (q.has_plane) {
            bool far = false, inl = false;
            if (has[k]) {
                far = far_from_plane(c.Tinv, q.coeffs, c.roadDistThr, {px[k], py[k], pz[k]});
                inl = mask_bit(mw[k], orig[k]);  // (the word was loaded with the point)
            }
            mi = __ballot(inl);
            mf = __ballot(far);
            n_inl += (int)__popcll(mi);
            n_far += (int)__popcll(mf);
        }
        if (lane == 0) {
            plane_row(planes, c, s, 0, ys[k])[wxs[k]] = mo;
            if (q.has_plane) {
                plane_row(planes, c, s, 1, ys[k])[wxs[k]] = mi;
                plane_row(planes, c, s, 2, ys[k])[wxs[k]] = mf;
            }
        }
    }
    const bool bad = __ballot(badl) != 0ull;
    if (lane == 0) {
        wsum[w][0] = n_occ;
        wsum[w][1] = n_inl;
        wsum[w][2] = n_far;
        wsum[w][3] = bad ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) t += wsum[k][threadIdx.x];
        as_global(partA)[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
    }
}

// Grid: n_seq * strips * bands blocks; a thread per column of the tile.  Dynamic LDS: the words of the bit planes the tile
// reaches (3 x tileRows x 6, behind the prefix), and the prefix, tileRows x 256 entries
// of 4 x 16 bits (narrow occupied | wide occupied << 16 | wide inlier << 32 | wide far << 48).  A prefix entry sums at
// most tileRows - 1 <= kMaxBand + 63 rows of at most 64 cells: below 2^16.  partB: per block (pixels with bit 0, pixels
// with bit 1, largest n_nb, 0).  nbfull: per pixel 0 without bit 0, else n_nb + 1 (written only when the call has buckets).
__global__ __launch_bounds__(kBlock) void k_coverage_count(const CvSeq* __restrict__ desc, CvCalib c, CvCall call,
                                                           unsigned long long* planes, int32_t* partB, uint16_t* nbfull) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long prefix[];
    __shared__ int rows_lo1[kMaxBand], rows_hi1[kMaxBand], rows_lo2[kMaxBand], rows_hi2[kMaxBand];
    __shared__ int wsum[kWaves][3];
    const int per_seq = c.strips * c.bands;
    const int s = (int)(blockIdx.x / (unsigned)per_seq), rem = (int)(blockIdx.x % (unsigned)per_seq);
    const int band = rem / c.strips, strip = rem - band * c.strips;
    const CvSeq q = desc[s];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int x = strip * kBlock + tid;
    const int ya = band * c.BR;
    const int nrows = min(c.BR, c.H - ya);
    // the row bounds of the band, once per block
    if (tid < nrows) {
        int lo, hi;
        window_bounds(ya + tid, c.halfY1, c.H - 1, lo, hi);
        rows_lo1[tid] = lo, rows_hi1[tid] = hi;
        window_bounds(ya + tid, c.halfY2, c.H - 1, lo, hi);
        rows_lo2[tid] = lo, rows_hi2[tid] = hi;
    }
    __syncthreads();
    const int r0 = rows_lo2[0], r1 = rows_hi2[nrows - 1];  // the rows of the tile: the band and its halo
    // the words of the bit planes the tile's windows reach: those of the wide windows of its first and its last column
    int lo_, hi_;
    window_bounds(strip * kBlock, c.halfX2, c.W - 1, lo_, hi_);
    const int wfirst = lo_ >> 6;
    window_bounds(min(c.W - 1, strip * kBlock + kBlock - 1), c.halfX2, c.W - 1, lo_, hi_);
    const int nW = (hi_ >> 6) - wfirst + 1;
    const int ntile = r1 - r0 + 1;
    const bool fits = r0 >= 0 && r1 < c.H && ntile + 1 <= c.tileRows && nW >= 1 && nW <= kStageWords;  // (always: what create checked)
    const bool in = x < c.W && fits;
    const bool plane = q.has_plane != 0;
    // the column bounds, once per thread
    ColSpan s1 = {0, 0, 0ull, 0ull}, s2 = s1;
    if (in) {
        int lo, hi;
        window_bounds(x, c.halfX1, c.W - 1, lo, hi);
        s1 = col_span(lo, hi);
        window_bounds(x, c.halfX2, c.W - 1, lo, hi);
        s2 = col_span(lo, hi);
    }
    unsigned long long* stage = prefix + (size_t)c.tileRows * kBlock;  // [plane][row of the tile][kStageWords]
    if (fits) {  // one coalesced pass over the tile's words instead of loads from global memory in the row loop
        const int per_plane = ntile * nW, total = (plane ? 3 : 1) * per_plane;
        for (int i = tid; i < total; i += kBlock) {
            const int p = i / per_plane, j = i - p * per_plane;
            const int rr = j / nW, ww = j - rr * nW;
            stage[((size_t)p * c.tileRows + rr) * kStageWords + ww] = plane_row(planes, c, s, p, r0 + rr)[wfirst + ww];
        }
    }
    __syncthreads();
    if (in) {
        s1.w0 -= wfirst, s1.w1 -= wfirst, s2.w0 -= wfirst, s2.w1 -= wfirst;
        unsigned long long run = 0ull;
        prefix[tid] = 0ull;
        for (int rr = 0; rr < ntile; rr++) {
            const unsigned long long* occ = stage + (size_t)rr * kStageWords;
            unsigned long long h = (unsigned long long)span_count(occ, s1) | ((unsigned long long)span_count(occ, s2) << 16);
            if (plane) {
                h |= (unsigned long long)span_count(occ + (size_t)c.tileRows * kStageWords, s2) << 32;
                h |= (unsigned long long)span_count(occ + (size_t)2 * c.tileRows * kStageWords, s2) << 48;
            }
            run += h;
            prefix[(size_t)(rr + 1) * kBlock + tid] = run;
        }
    }
    __syncthreads();  // (a thread reads its own column only; the barrier orders the LDS writes before the reads all the same)
    int n_bit0 = 0, n_bit1 = 0, top_nb = 0;
    if (in) {
        MLD_BATCH_GLOBAL uint8_t* o_nb = as_global(q.nb);
        MLD_BATCH_GLOBAL uint8_t* o_road = as_global(q.road);
        MLD_BATCH_GLOBAL uint8_t* o_inl = as_global(q.road_inl);
        MLD_BATCH_GLOBAL uint8_t* o_far = as_global(q.road_far);
        MLD_BATCH_GLOBAL uint8_t* o_reach = as_global(q.reach);
        MLD_BATCH_GLOBAL uint16_t* o_full = as_global(nbfull) + (size_t)s * (size_t)c.W * (size_t)c.H;
        for (int i = 0; i < nrows; i++) {
            const unsigned long long n1 = prefix[(size_t)(rows_hi1[i] - r0 + 1) * kBlock + tid] - prefix[(size_t)(rows_lo1[i] - r0) * kBlock + tid];
            const unsigned long long n2 = prefix[(size_t)(rows_hi2[i] - r0 + 1) * kBlock + tid] - prefix[(size_t)(rows_lo2[i] - r0) * kBlock + tid];
            const int n_nb = (int)(n1 & 0xffffull);
            const int n_road = (int)((n2 >> 16) & 0xffffull), n_inl = (int)((n2 >> 32) & 0xffffull), n_far = (int)(n2 >> 48);
            // DepthEstimator.cpp:680 and :585, compared as unsigned; :814-815 no far neighbour; :827 three inliers
            const bool bit0 = !c.allZero && (unsigned)n_nb >= c.countMin;
            const bool bit1 = bit0 && plane && (unsigned)n_road >= c.countMin && n_far == 0 && n_inl >= 3;
            const size_t at = (size_t)x + (size_t)(ya + i) * (size_t)c.W;
            if (o_nb) o_nb[at] = (uint8_t)min(n_nb, 255);
            if (o_road) o_road[at] = (uint8_t)min(n_road, 255);
            if (o_inl) o_inl[at] = (uint8_t)min(n_inl, 255);
            if (o_far) o_far[at] = (uint8_t)min(n_far, 255);
            if (o_reach) o_reach[at] = (uint8_t)((bit0 ? 1 : 0) | (bit1 ? 2 : 0));
            if (call.bucket_w) o_full[at] = (uint16_t)(bit0 ? n_nb + 1 : 0);
            n_bit0 += bit0 ? 1 : 0;
            n_bit1 += bit1 ? 1 : 0;
            top_nb = max(top_nb, n_nb);
        }
    }
    n_bit0 = wave_sum(n_bit0);
    n_bit1 = wave_sum(n_bit1);
    top_nb = wave_max(top_nb);
    if (lane == 0) {
        wsum[w][0] = n_bit0;
        wsum[w][1] = n_bit1;
        wsum[w][2] = top_nb;
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0, m = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            a += wsum[k][0];
            b += wsum[k][1];
            m = max(m, wsum[k][2]);
        }
        MLD_BATCH_GLOBAL int32_t* out = as_global(partB) + (size_t)blockIdx.x * 4;
        out[0] = a;
        out[1] = b;
        out[2] = m;
        out[3] = 0;
    }
}

// Grid: n_seq * per_seq blocks, per_seq = 1 + ceil(buckets / 4).  Block 0 of a sequence sums the block partials into the
// record; the wavefronts of the others take one bucket each: the largest (n_nb, then smallest y, then smallest x) among
// the pixels with bit 0, as the largest key (n_nb + 1) << 32 | (2^31 - 1 - (x + y * W)).
__global__ __launch_bounds__(kBlock) void k_coverage_finish(const CvSeq* __restrict__ desc, CvCalib c, CvCall call, const int32_t* partA,
                                                            const int32_t* partB, const uint16_t* nbfull, int per_seq) {
    __shared__ long long sums[kWaves][5];
    __shared__ int tops[kWaves][2];
    const int s = (int)(blockIdx.x / (unsigned)per_seq), blk = (int)(blockIdx.x % (unsigned)per_seq);
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    if (blk == 0) {
        long long v[5] = {0, 0, 0, 0, 0};
        int top = 0, bad = 0;
        const MLD_BATCH_GLOBAL int32_t* pa = as_global(partA) + (size_t)s * (size_t)c.blocksA * 4;
        for (int i = tid; i < c.blocksA; i += kBlock) {
            v[2] += pa[4 * (size_t)i];
            v[3] += pa[4 * (size_t)i + 1];
            v[4] += pa[4 * (size_t)i + 2];
            bad |= pa[4 * (size_t)i + 3];
        }
        const int nb = c.strips * c.bands;
        const MLD_BATCH_GLOBAL int32_t* pb = as_global(partB) + (size_t)s * (size_t)nb * 4;
        for (int i = tid; i < nb; i += kBlock) {
            v[0] += pb[4 * (size_t)i];
            v[1] += pb[4 * (size_t)i + 1];
            top = max(top, pb[4 * (size_t)i + 2]);
        }
#pragma unroll
        for (int k = 0; k < 5; k++) {
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
        }
        top = wave_max(top);
        bad = wave_max(bad);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 5; k++) sums[w][k] = v[k];
            tops[w][0] = top;
            tops[w][1] = bad;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < kWaves; k++) {
                for (int j = 0; j < 5; j++) sums[0][j] += sums[k][j];
                tops[0][0] = max(tops[0][0], tops[k][0]);
                tops[0][1] |= tops[k][1];
            }
            MLD_BATCH_GLOBAL mld_coverage_record* rec = as_global(call.record) + s;
            rec->n_reach = sums[0][0];
            rec->n_reach_road = sums[0][1];
            rec->n_occupied = sums[0][2];
            rec->n_inlier = sums[0][3];
            rec->n_far = sums[0][4];
            rec->max_nb = tops[0][0];
            rec->flags = (tops[0][1] ? MLD_COVERAGE_FLAG_BAD_INPUT : 0) | (desc[s].has_plane ? MLD_COVERAGE_FLAG_HAS_PLANE : 0);
            rec->n_buckets = call.nbx * call.nby;
            rec->pad_[0] = rec->pad_[1] = rec->pad_[2] = 0;
        }
        return;
    }
    const CvSeq q = desc[s];
    const long long b = (long long)(blk - 1) * kWaves + w;  // (uniform in the wavefront)
    if (b >= (long long)call.nbx * (long long)call.nby || b >= (long long)q.bucket_cap || !q.bucket) return;
    const int by = (int)(b / call.nbx), bx = (int)(b - (long long)by * call.nbx);
    const int xa = bx * call.bucket_w, yb0 = by * call.bucket_h;  // (inside the image: below 65536 each)
    const int wx = min(call.bucket_w, c.W - xa), hy = min(call.bucket_h, c.H - yb0);
    const int cells = wx * hy;  // (at most the image: 2^30)
    const MLD_BATCH_GLOBAL uint16_t* full = as_global(nbfull) + (size_t)s * (size_t)c.W * (size_t)c.H;
    long long best = 0;
    for (int i = lane; i < cells; i += kWave) {
        const int yy = i / wx, xx = i - yy * wx;
        const int at = (xa + xx) + (yb0 + yy) * c.W;
        const long long n1 = (long long)full[at];
        const long long key = n1 ? ((n1 << 32) | (long long)(0x7fffffff - at)) : 0ll;
        best = key > best ? key : best;
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(best, d);
        best = o > best ? o : best;
    }
    if (lane < 3) {
        int v;
        if (best == 0) {
            v = lane == 2 ? 0 : -1;
        } else {
            const int at = 0x7fffffff - (int)(best & 0xffffffffll);
            const int py = at / c.W, px = at - py * c.W;
            v = lane == 0 ? px : (lane == 1 ? py : (int)(best >> 32) - 1);
        }
        as_global(q.bucket)[3 * (size_t)b + lane] = v;
    }
}

char g_error[512] = "";  // refusals without an object: mld_coverage_maps_last_error(NULL)

// Dynamic LDS of k_coverage_count: the prefix and the staged words of three bit planes.
size_t lds_bytes(int tile_rows) { return (size_t)tile_rows * (kBlock + 3 * kStageWords) * sizeof(unsigned long long); }

// What mld_create refuses of a parameter set, a camera and a transform that bears on the neighbour stage, with its texts;
// and what only this object refuses.
int refuse_config(const mld_params& P, const mld_camera& cam, const double T[12], std::string& why) {
    int code = refuse_modes(P, why);
    if (code == MLD_OK) code = refuse_window_and_image(P, cam, why);  // (the intrinsics play no part in the neighbour stage)
    if (code == MLD_OK) code = refuse_transform(T, why);
    if (code != MLD_OK) return code;
    double halfX1, halfY1, halfX2, halfY2;
    window_halves(P, halfX1, halfY1, halfX2, halfY2);
    if (window_span(halfX2, cam.width) > kMaxSpan || window_span(halfY2, cam.height) > kMaxSpan) {
        why = "the wide window (2.0 x 1.5 the search area) can span more than 64 columns or more than 64 rows";
        return MLD_ERR_CAPACITY;
    }
    return MLD_OK;
}

void build_calib(CvCalib& c, const mld_params& P, const mld_camera& cam, const double T[12]) {
    camera_to_lidar(T, c.Tinv);
    c.W = cam.width;
    c.H = cam.height;
    c.WW = (cam.width + 63) / 64;
    window_halves(P, c.halfX1, c.halfY1, c.halfX2, c.halfY2);
    c.countMin = (unsigned)P.radiusSearch_count_min;
    c.allZero = P.set_all_depths_to_zero ? 1 : 0;
    c.roadDistThr = P.ransac_plane_point_distance_treshold;
    const int span = window_span(c.halfY2, cam.height);
    c.BR = span <= 16 ? kMaxBand : kMaxBand / 2;  // (a tall window: a shorter band, so that the prefix stays within LDS)
    c.tileRows = c.BR + span;                     // BR - 1 + span rows of the tile at most, and the zero row
    c.blocksA = (int)(((int64_t)c.WW * c.H + kWordsPerBlock - 1) / kWordsPerBlock);
    c.strips = (cam.width + kBlock - 1) / kBlock;
    c.bands = (cam.height + c.BR - 1) / c.BR;
}

}  // namespace

struct mld_coverage_maps : mld_batch::Object {
    int n_seq = 0;
    int use_road = 0;
    CvCalib calib{};
    size_t lds_bytes = 0;
    mld_batch::DeviceBuffer<unsigned long long> d_planes;  // n_seq x 3 x H x WW words
    mld_batch::DeviceBuffer<int32_t> d_partA;              // n_seq x blocksA x 4
    mld_batch::DeviceBuffer<int32_t> d_partB;              // n_seq x strips x bands x 4
    mld_batch::DeviceBuffer<uint16_t> d_nbfull;            // n_seq x W x H: the bucket partials
    mld_batch::DescRing<CvSeq> ring;
};

extern "C" {

mld_coverage_maps* mld_coverage_maps_create(mld_ctx* ctx, int n_seq, const mld_params* params, const mld_camera* camera,
                                            const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the size first: it is refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_coverage_maps_create: n_seq must be in 1 .. 65536";
        if (!ctx) return "mld_coverage_maps_create: null context";
        if (!params) return "mld_coverage_maps_create: null params";
        if (!camera) return "mld_coverage_maps_create: null camera";
        if (!T_cam_lidar) return "mld_coverage_maps_create: null T_cam_lidar";
        return nullptr;
    };
    const char* bad = refusal();
    std::string why;
    int code = MLD_OK;
    if (!bad) {  // (what is refused with a status of its own; still nothing of the context is used)
        code = refuse_config(*params, *camera, T_cam_lidar, why);
        if (code == MLD_OK) {
            CvCalib c{};
            build_calib(c, *params, *camera, T_cam_lidar);
            const int64_t most = c.blocksA > c.strips * c.bands ? c.blocksA : c.strips * c.bands;
            if ((int64_t)n_seq * most > kMaxGrid) {
                why = "n_seq sequences of this image size need more than 2^31 - 1 blocks";
                code = MLD_ERR_CAPACITY;
            }
        }
    }
    auto init = [&](mld_coverage_maps* cm) -> int {
        cm->n_seq = n_seq;
        cm->use_road = params->do_use_ransac_plane ? 1 : 0;
        build_calib(cm->calib, *params, *camera, T_cam_lidar);
        const CvCalib& c = cm->calib;
        cm->lds_bytes = lds_bytes(c.tileRows);
        // More dynamic LDS than a kernel gets unasked.  Every object asks for the same figure, the most any object can
        // need, so that objects do not lower one another's.
        MLD_HIP(cm, hipFuncSetAttribute(reinterpret_cast<const void*>(k_coverage_count), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds_bytes(kMaxBand / 2 + kMaxSpan)));
        const size_t S = (size_t)n_seq;
        int rc;
        if ((rc = cm->d_planes.allocate(cm, S * 3 * (size_t)c.H * (size_t)c.WW))) return rc;
        if ((rc = cm->d_partA.allocate(cm, S * (size_t)c.blocksA * 4))) return rc;
        if ((rc = cm->d_partB.allocate(cm, S * (size_t)c.strips * (size_t)c.bands * 4))) return rc;
        if ((rc = cm->d_nbfull.allocate(cm, S * (size_t)c.W * (size_t)c.H))) return rc;
        return cm->ring.allocate(cm, n_seq);
    };
    return mld_batch::create_object<mld_coverage_maps>(g_error, "mld_coverage_maps_create", bad, ctx, status_out, init, code,
                                                       why.c_str());
}

void mld_coverage_maps_destroy(mld_coverage_maps* cm) { mld_batch::destroy_object(cm); }

const char* mld_coverage_maps_last_error(const mld_coverage_maps* cm) { return cm ? cm->err.c_str() : g_error; }

int mld_coverage_maps_collect_device(mld_coverage_maps* cm, const int32_t* const* map, const int32_t* const* index,
                                     const int64_t* index_len, const double* const* cam, const int64_t* n_points, const float* coeffs,
                                     const uint32_t* const* mask_dev, uint8_t* const* nb_out, uint8_t* const* road_out,
                                     uint8_t* const* road_inl_out, uint8_t* const* road_far_out, uint8_t* const* reach_out,
                                     mld_coverage_record* record_out_dev, int bucket_w, int bucket_h, const int64_t* bucket_capacity,
                                     int32_t* const* bucket_out) {
    const char* fn = "mld_coverage_maps_collect_device";
    if (!cm) return no_object(g_error, fn, "cm");
    auto refuse = [&](int code, const char* text) { return fail(cm, code, (std::string(fn) + ": " + text).c_str()); };
#define CV_REFUSE(text) return refuse(MLD_ERR_INVALID_ARG, text)
    if (!map) CV_REFUSE("null table map");
    if (!index) CV_REFUSE("null table index");
    if (!index_len) CV_REFUSE("null table index_len");
    if (!cam) CV_REFUSE("null table cam");
    if (!n_points) CV_REFUSE("null table n_points");
    if (!record_out_dev) CV_REFUSE("null array record_out_dev");
    if (misaligned(record_out_dev, 7u)) CV_REFUSE("record_out_dev must be 8-byte aligned");
    if ((coeffs != nullptr) != (mask_dev != nullptr)) CV_REFUSE("coeffs and mask_dev come together or not at all");
    if (bucket_out) {
        if (bucket_w < 1 || bucket_w > 65535 || bucket_h < 1 || bucket_h > 65535) CV_REFUSE("bucket_w and bucket_h must be in 1 .. 65535");
        if (!bucket_capacity) CV_REFUSE("null table bucket_capacity");
    }
    const int S = cm->n_seq;
    const CvCalib& c = cm->calib;
    CvCall call{};
    call.record = record_out_dev;
    if (bucket_out) {
        call.bucket_w = bucket_w;
        call.bucket_h = bucket_h;
        call.nbx = (c.W + bucket_w - 1) / bucket_w;
        call.nby = (c.H + bucket_h - 1) / bucket_h;
    }
    const int64_t n_buckets = (int64_t)call.nbx * call.nby;
    const int64_t per_seq = 1 + (n_buckets + kWaves - 1) / kWaves;
    for (int s = 0; s < S; s++) {
        if (index_len[s] < 0) CV_REFUSE("negative index_len");
        if (n_points[s] < 0) CV_REFUSE("negative n_points");
        if (bucket_out && bucket_capacity[s] < 0) CV_REFUSE("negative bucket_capacity");
        if (n_points[s] > kMaxPoints || index_len[s] > kMaxPoints) return refuse(MLD_ERR_CAPACITY, "n_points or index_len exceeds 8 388 607");
        if (!map[s]) CV_REFUSE("null array map");
        if (index_len[s] > 0 && !index[s]) CV_REFUSE("null array index of a sequence with index_len > 0");
        if (n_points[s] > 0 && !cam[s]) CV_REFUSE("null array cam of a sequence with n_points > 0");
        if (bucket_out && bucket_capacity[s] > 0 && !bucket_out[s]) CV_REFUSE("null array bucket_out of a sequence with bucket_capacity > 0");
        if (misaligned(map[s], 3u)) CV_REFUSE("map must be 4-byte aligned");
        if (misaligned(index[s], 3u)) CV_REFUSE("index must be 4-byte aligned");
        if (misaligned(cam[s], 7u)) CV_REFUSE("cam must be 8-byte aligned");
        if (mask_dev && misaligned(mask_dev[s], 3u)) CV_REFUSE("mask_dev must be 4-byte aligned");
        if (bucket_out && misaligned(bucket_out[s], 3u)) CV_REFUSE("bucket_out must be 4-byte aligned");
    }
    if ((int64_t)S * per_seq > kMaxGrid) return refuse(MLD_ERR_CAPACITY, "buckets this small need more than 2^31 - 1 blocks");
#undef CV_REFUSE
    for (int s = 0; s < S; s++) {
        CvSeq& q = cm->ring.stage[(size_t)s];
        q = CvSeq{};
        q.map = map[s];
        q.index = index[s];
        q.cam = cam[s];
        q.has_plane = (cm->use_road && coeffs && mask_dev && mask_dev[s]) ? 1 : 0;
        q.mask = q.has_plane ? mask_dev[s] : nullptr;
        q.nb = nb_out ? nb_out[s] : nullptr;
        q.road = road_out ? road_out[s] : nullptr;
        q.road_inl = road_inl_out ? road_inl_out[s] : nullptr;
        q.road_far = road_far_out ? road_far_out[s] : nullptr;
        q.reach = reach_out ? reach_out[s] : nullptr;
        q.bucket = bucket_out ? bucket_out[s] : nullptr;
        for (int t = 0; t < 4; t++) q.coeffs[t] = q.has_plane ? coeffs[4 * (size_t)s + t] : 0.f;
        q.index_len = (int32_t)index_len[s];
        q.n_points = (int32_t)n_points[s];
        const int64_t cap = (bucket_out && q.bucket) ? bucket_capacity[s] : 0;
        q.bucket_cap = (int32_t)(cap < n_buckets ? cap : n_buckets);
    }
    MLD_HIP(cm, hipSetDevice(cm->device));
    const int rc = cm->ring.upload(cm);
    if (rc) return rc;
    hipLaunchKernelGGL(k_coverage_classify, dim3((unsigned)((int64_t)S * c.blocksA)), dim3(kBlock), 0, cm->stream, cm->ring.d_desc.get(), c,
                       cm->d_planes.get(), cm->d_partA.get());
    MLD_HIP(cm, hipGetLastError());
    hipLaunchKernelGGL(k_coverage_count, dim3((unsigned)((int64_t)S * c.strips * c.bands)), dim3(kBlock), cm->lds_bytes, cm->stream,
                       cm->ring.d_desc.get(), c, call, cm->d_planes.get(), cm->d_partB.get(), cm->d_nbfull.get());
    MLD_HIP(cm, hipGetLastError());
    hipLaunchKernelGGL(k_coverage_finish, dim3((unsigned)((int64_t)S * per_seq)), dim3(kBlock), 0, cm->stream, cm->ring.d_desc.get(), c, call,
                       cm->d_partA.get(), cm->d_partB.get(), cm->d_nbfull.get(), (int)per_seq);
    MLD_HIP(cm, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
