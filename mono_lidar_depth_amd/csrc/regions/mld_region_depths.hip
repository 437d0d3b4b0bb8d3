// mld_region_depths.hip — the foreground depth of image rectangles, for a batch of sequences in one call (include/mld.h,
// "mld_region_depths"): the window scan of NeighborFinderPixel::getNeighbors (NeighborFinderPixel.cpp:70-79) over a box of
// ANY size, the first-local-maximum histogram of PointHistogram::FilterPointsMinDistBlob (HistogramPointDepth.cpp:30-100)
// with the binning of Histogram::AddElement (Histogram.cpp:29-30), and count, minimum, maximum, exact median and nearest
// point of the box.  The inputs are the arrays mld_projected_clouds_export_device writes (pixel map, _pointIndex,
// camera-frame cloud) and, optionally, the inlier bitmask the plane objects leave on the device.  The record holds only
// counts, order statistics and bin borders: nothing here accumulates in floating point, and the only atomics are integer
// adds in LDS, whose sums do not depend on their order.
//
// Two launches: the descriptor upload and
//   k_region_depths   one block per box.  Scan 1 walks the clipped box in row-major order - thread t takes the cells t,
//                     t + 256, ...; eight cells per thread are in flight, their loads issued in stages (map, index, z and
//                     mask word) - and reduces count, ground count, bad input, the largest z and the smallest (z, scan
//                     position) with the point's original index.  The z of the counted points go into a list in LDS while
//                     they fit (kListCap).  Then, from the list or - for a box with more counted points - from further
//                     scans of the box: step 0 fills the histogram (kHistBins bins from the bin of z_min on) and the first
//                     radix pass of the median, step 1 counts the points inside the chosen bin and runs the second radix
//                     pass, further steps the remaining radix passes.  A radix pass histograms 8 bits of the bit pattern
//                     of z among the values that share the bits chosen so far; the passes start at the highest bit in which
//                     z_min and z_max differ.  A re-scanning box stops scanning as soon as it can: from step 1 on, once
//                     the values that still share the chosen bits fit the list, the scan of that step also collects them
//                     there, and the remaining passes run on the list.  Both routes run the same steps on the same
//                     values, so the record is the same bit for bit.
// A box without a counted point leaves after scan 1; a box of one distinct value needs no radix pass.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, lane_rank, wave_sum and the size limits:
// ../batch/mld_batch_device.h), and it is compiled without contraction like the rest of the library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"
#include "../../../include/mld.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;  // threads of a block
constexpr int kWaves = kBlock / kWave;
constexpr int kCells = 8;    // cells of a thread in flight
constexpr int kListCap = MLD_REGION_LIST_CAPACITY;
constexpr int kHistBins = MLD_REGION_HIST_BINS;
constexpr int kRadix = 256;  // 8 bits a pass
constexpr int64_t kMaxGrid = 2147483647;
constexpr unsigned long long kNoKey = ~0ull;

static_assert(sizeof(mld_region_depth) == 80, "80 bytes per record (include/mld.h)");
static_assert(offsetof(mld_region_depth, nearest_orig) == 16 && offsetof(mld_region_depth, clip) == 20 &&
                  offsetof(mld_region_depth, z_min) == 40 && offsetof(mld_region_depth, hist_lower) == 64,
              "field offsets of the record (include/mld.h)");
static_assert(kRadix == kBlock && kHistBins % kBlock == 0, "a thread clears one radix bin and kHistBins / kBlock histogram bins");
// 16 KiB of list, 2 KiB of histogram, 1 KiB of radix bins and the partials: the 160 KiB of LDS of a CU would hold eight
// blocks; the registers (93 VGPRs) hold five, 20 of a CU's 32 wavefronts.

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct RgSeq {
    const int32_t* map;        // W * H: visible index or -1
    const int32_t* index;      // index_len: original index of a visible point
    const double* cam;         // 3 x n_points
    const uint32_t* mask;      // ceil(n_points / 32) words, or null
    const int32_t* boxes;      // n_boxes x 4
    mld_region_depth* record;  // n_boxes
    int32_t index_len;
    int32_t n_points;
    int32_t n_boxes;
    int32_t pad_;
};
static_assert(sizeof(RgSeq) == 64, "64 bytes per sequence (include/mld.h, DESIGN.md)");

struct RgCalib {
    double binW;       // histogram_segmentation_bin_witdh
    int32_t minCount;  // histogram_segmentation_min_pointcount
    int32_t W, H;
    int32_t listCap;   // kListCap (the A/B library: what the environment asks for)
};

// The clipped box of a block and the step of a thread from one of its cells to the next (kBlock cells on).
struct Geo {
    int x0, y0, bw, cells;
    int dx, dy;  // kBlock = dy * bw + dx
};

// The position in the box of a thread's next cell.
struct Cursor {
    int x, y;
};

__device__ __forceinline__ Cursor cursor_at(const Geo& g, int tid) {
    Cursor c;
    c.y = tid / g.bw;
    c.x = tid - c.y * g.bw;
    return c;
}

// kCells cells of a thread: base + tid, base + kBlock + tid, ...  state: 1 counted, 2 ground, 0 nothing; zb: the bits of z.
struct Batch {
    unsigned long long zb[kCells];
    int orig[kCells];
    int state[kCells];
};

// The loads in stages - every map value, then every index, then every z and mask word - so that a wavefront waits for
// three loads in a row and not for three per cell.  Returns whether a cell was bad input.
__device__ __forceinline__ bool fetch(const RgSeq& q, int W, const Geo& g, int base, int tid, Cursor& cur, Batch& b) {
    const MLD_BATCH_GLOBAL int32_t* map = as_global(q.map);
    const MLD_BATCH_GLOBAL int32_t* index = as_global(q.index);
    const MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    const MLD_BATCH_GLOBAL uint32_t* mask = as_global(q.mask);
    bool bad = false;
    int m[kCells];
#pragma unroll
    for (int k = 0; k < kCells; k++) {
        const int i = base + k * kBlock + tid;
        m[k] = (i < g.cells) ? map[(size_t)(g.x0 + cur.x) + (size_t)(g.y0 + cur.y) * (size_t)W] : -1;
        cur.x += g.dx;
        cur.y += g.dy;
        if (cur.x >= g.bw) {
            cur.x -= g.bw;
            cur.y++;
        }
    }
#pragma unroll
    for (int k = 0; k < kCells; k++) {
        const bool in_index = m[k] >= 0 && m[k] < q.index_len;
        if (m[k] != -1 && !in_index) bad = true;
        b.orig[k] = in_index ? index[m[k]] : -1;
    }
    uint32_t mw[kCells];
#pragma unroll
    for (int k = 0; k < kCells; k++) {
        const bool in_index = m[k] >= 0 && m[k] < q.index_len;
        const bool has = in_index && b.orig[k] >= 0 && b.orig[k] < q.n_points;
        if (in_index && !has) bad = true;
        b.zb[k] = 0ull;
        mw[k] = 0u;
        b.state[k] = has ? 1 : 0;
        if (has) {
            b.zb[k] = (unsigned long long)__double_as_longlong(cam[3 * (size_t)b.orig[k] + 2]);
            if (mask) mw[k] = mask[(unsigned)b.orig[k] >> 5];
        }
    }
#pragma unroll
    for (int k = 0; k < kCells; k++) {
        if (b.state[k]) {
            if (!(__longlong_as_double((long long)b.zb[k]) > 0.0)) {  // zero, negative, NaN
                bad = true;
                b.state[k] = 0;
            } else if ((mw[k] >> ((unsigned)b.orig[k] & 31u)) & 1u) {
                b.state[k] = 2;
            }
        }
    }
    return bad;
}

// f(bits of z) for every counted point of the box: from the list in LDS, or by another scan.
template <typename F>
__device__ __forceinline__ void for_each_z(bool listed, const unsigned long long* list, int n, const RgSeq& q, int W, const Geo& g, int tid,
                                           F f) {
    if (listed) {
        for (int j = tid; j < n; j += kBlock) f(list[j]);
        return;
    }
    Cursor cur = cursor_at(g, tid);
    Batch b;
    for (int base = 0; base < g.cells; base += kCells * kBlock) {
        (void)fetch(q, W, g, base, tid, cur, b);
#pragma unroll
        for (int k = 0; k < kCells; k++)
            if (b.state[k] == 1) f(b.zb[k]);
    }
}

// Histogram.cpp:29-30 for a bin count as a double.
__device__ __forceinline__ int bin_of(double z, double binW, double lim) {
    const double value = (1e10 < z) ? 1e10 : z;
    const double qd = fabs(value / binW);
    return (int)((lim < qd) ? lim : qd);
}

// Grid: n_seq * per_seq blocks, block b of a sequence its box b.
__global__ __launch_bounds__(kBlock) void k_region_depths(const RgSeq* __restrict__ desc, RgCalib c, int per_seq) {
    __shared__ unsigned long long list[kListCap];
    __shared__ int hist[kHistBins];
    __shared__ int rad[kRadix];
    __shared__ unsigned long long w_key[kWaves], w_max[kWaves];
    __shared__ int w_pos[kWaves], w_orig[kWaves], w_cnt[kWaves][3];
    __shared__ int s_n, s_seg, s_digit, s_rank, s_cand, s_hist[2];  // s_hist: flags of the rule, the chosen bin
    const int s = (int)(blockIdx.x / (unsigned)per_seq), bi = (int)(blockIdx.x % (unsigned)per_seq);
    const RgSeq q = desc[s];
    if (bi >= q.n_boxes) return;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    MLD_BATCH_GLOBAL mld_region_depth* rec = as_global(q.record) + bi;
    const MLD_BATCH_GLOBAL int32_t* box = as_global(q.boxes) + 4 * (size_t)bi;
    const int bx0 = box[0], by0 = box[1], bx1 = box[2], by1 = box[3];
    // NeighborFinderPixel.cpp:70-79 for integer edges: max(x0, 0), min(x1, W - 1), both scanned inclusive
    const int cx0 = max(bx0, 0), cy0 = max(by0, 0), cx1 = min(bx1, c.W - 1), cy1 = min(by1, c.H - 1);
    const int mask_flag = q.mask ? MLD_REGION_FLAG_HAS_MASK : 0;
    const bool empty = bx1 < bx0 || by1 < by0 || cx1 < cx0 || cy1 < cy0;
    Geo g;
    g.x0 = cx0, g.y0 = cy0;
    g.bw = empty ? 1 : cx1 - cx0 + 1;
    g.cells = empty ? 0 : g.bw * (cy1 - cy0 + 1);  // (at most the image: 2^30)
    g.dy = kBlock / g.bw;
    g.dx = kBlock - g.dy * g.bw;

    // ---- scan 1: counts, extremes, nearest point, the list
    if (tid == 0) s_n = 0, s_seg = 0;
#pragma unroll
    for (int k = 0; k < kHistBins / kBlock; k++) hist[k * kBlock + tid] = 0;
    rad[tid] = 0;
    __syncthreads();
    int cnt = 0, ground = 0, pos = 0, orig = -1;
    bool badl = false;
    unsigned long long key = kNoKey, top = 0ull;
    {
        Cursor cur = cursor_at(g, tid);
        Batch b;
        for (int base = 0; base < g.cells; base += kCells * kBlock) {  // (uniform in the block)
            if (fetch(q, c.W, g, base, tid, cur, b)) badl = true;
#pragma unroll
            for (int k = 0; k < kCells; k++) {
                const bool counted = b.state[k] == 1;
                ground += b.state[k] == 2 ? 1 : 0;
                if (counted) {
                    cnt++;
                    if (b.zb[k] < key) {  // (a thread's cells come in scan order: the first of equal z stays)
                        key = b.zb[k];
                        pos = base + k * kBlock + tid;
                        orig = b.orig[k];
                    }
                    top = b.zb[k] > top ? b.zb[k] : top;
                }
                if (c.listCap > 0) {
                    const unsigned long long m = __ballot(counted);
                    if (m != 0ull) {  // (uniform in the wavefront)
                        int at = 0;
                        if (lane == 0) at = atomicAdd(&s_n, (int)__popcll(m));
                        at = __shfl(at, 0) + lane_rank((unsigned)m, (unsigned)(m >> 32));
                        if (counted && at < c.listCap) list[at] = b.zb[k];
                    }
                }
            }
        }
    }
    cnt = wave_sum(cnt);
    ground = wave_sum(ground);
    const int badw = __ballot(badl) != 0ull ? 1 : 0;
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const unsigned long long ok = __shfl_xor(key, d), ot = __shfl_xor(top, d);
        const int op = __shfl_xor(pos, d), oo = __shfl_xor(orig, d);
        if (ok < key || (ok == key && op < pos)) key = ok, pos = op, orig = oo;
        top = ot > top ? ot : top;
    }
    if (lane == 0) {
        w_key[w] = key, w_max[w] = top, w_pos[w] = pos, w_orig[w] = orig;
        w_cnt[w][0] = cnt, w_cnt[w][1] = ground, w_cnt[w][2] = badw;
    }
    __syncthreads();
    int n = 0, n_ground = 0, bad = 0;
    key = kNoKey, top = 0ull, pos = 0, orig = -1;
#pragma unroll
    for (int k = 0; k < kWaves; k++) {  // (every thread the same: uniform from here on)
        n += w_cnt[k][0], n_ground += w_cnt[k][1], bad |= w_cnt[k][2];
        if (w_key[k] < key || (w_key[k] == key && w_pos[k] < pos)) key = w_key[k], pos = w_pos[k], orig = w_orig[k];
        top = w_max[k] > top ? w_max[k] : top;
    }
    int flags = mask_flag | (bad ? MLD_REGION_FLAG_BAD_INPUT : 0) | (empty ? MLD_REGION_FLAG_EMPTY_BOX : 0);
    if (n == 0) {
        if (tid == 0) {
            rec->n_points = 0, rec->n_ground = n_ground, rec->n_seg = 0, rec->flags = flags, rec->nearest_orig = -1;
            rec->clip[0] = empty ? -1 : cx0, rec->clip[1] = empty ? -1 : cy0;
            rec->clip[2] = empty ? -1 : cx1, rec->clip[3] = empty ? -1 : cy1;
            rec->pad_ = 0;
            rec->z_min = rec->z_max = rec->z_median = -1.0;
            rec->hist_lower = rec->hist_higher = -1.0;
        }
        return;
    }
    const double z_min = __longlong_as_double((long long)key), z_max = __longlong_as_double((long long)top);
    const bool listed = n <= c.listCap;

    // ---- the histogram's frame (HistogramPointDepth.cpp:36-43,53), integers beyond the int range saturated
    const double up = ceil(z_max);
    const int maxDist = up >= 2147483648.0 ? 2147483647 : (int)up;
    const double bc = (double)maxDist / c.binW + 1.0;
    const int binCount = bc >= 2147483648.0 ? 2147483647 : (int)bc;
    const double lim = (double)binCount - 1.;
    const int b0 = bin_of(z_min, c.binW, lim);  // (the lowest bin with a point: bin_of does not decrease with z)

    // ---- the radix passes: 8 bits each, from the highest bit in which z_min and z_max differ
    const unsigned long long diff = key ^ top;
    const int passes = diff ? (64 - (int)__clzll((long long)diff) + 7) / 8 : 0;
    unsigned long long prefix = passes < 8 ? key >> (8 * passes) : 0ull;  // the bits above the passes: common to all
    int rank = (n - 1) / 2;
    double lower = -1.0, higher = -1.0;
    int n_seg = 0;
    bool from_list = listed;  // the values the next step looks at lie in the list
    int n_list = n;           // how many
    int cand = n;             // values that share the bits chosen so far
    const int steps = passes > 2 ? passes : 2;
    for (int step = 0; step < steps; step++) {  // (uniform)
        const bool do_hist = step == 0 && binCount > 1;
        const bool do_seg = step == 1 && (flags & MLD_REGION_FLAG_HIST_FOUND);
        const bool do_rad = step < passes;
        if (!(do_hist || do_seg || do_rad)) continue;
        const int p = passes - 1 - step;  // this pass's digit: bits 8p .. 8p + 7
        // the histogram is done (step 0) and n_seg is being done (step 1): a scan may keep what the later passes need
        const bool collect = !from_list && do_rad && step >= 1 && cand <= c.listCap;
        if (collect) {
            if (tid == 0) s_n = 0;
            __syncthreads();
        }
        int seg = 0;
        for_each_z(from_list, list, n_list, q, c.W, g, tid, [&](unsigned long long zb) {
            const double z = __longlong_as_double((long long)zb);
            if (do_hist) {
                const int r = bin_of(z, c.binW, lim) - b0;
                if (r >= 0 && r < kHistBins) atomicAdd(&hist[r], 1);
            }
            if (do_seg) seg += (z >= lower && z < higher) ? 1 : 0;
            if (do_rad && (p == 7 || (zb >> (8 * (p + 1))) == prefix)) {
                atomicAdd(&rad[(int)((zb >> (8 * p)) & 255ull)], 1);
                if (collect) {
                    const int at = atomicAdd(&s_n, 1);
                    if (at < kListCap) list[at] = zb;  // (cand of them: within the list)
                }
            }
        });
        if (do_seg) {
            seg = wave_sum(seg);
            if (lane == 0) atomicAdd(&s_seg, seg);
        }
        __syncthreads();
        if (do_rad && w == 0) {  // the digit that holds the rank: four bins per lane
            int cb[4], t = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) cb[k] = rad[4 * lane + k], t += cb[k];
            const int incl = scan_inclusive<kWave>(t, lane);
            int r = rank - (incl - t);
            if (r >= 0 && rank < incl) {  // (one lane)
                int d = 0;
                while (d < 3 && r >= cb[d]) r -= cb[d], d++;
                s_digit = 4 * lane + d;
                s_rank = r;
                s_cand = cb[d];
            }
        }
        if (do_hist && tid == kWave) {  // HistogramPointDepth.cpp:66-97 from bin b0 on: the empty bins ahead of it change nothing
            int binMaxId = -1, binMaxVal = -1, binValue = 0, verdict = 0;
            for (int i = b0; i < binCount; i++) {
                if (i - b0 >= kHistBins) {
                    verdict = MLD_REGION_FLAG_HIST_CAPPED;
                    break;
                }
                const int last = binValue;
                binValue = hist[i - b0];
                if ((binValue > binMaxVal) && (binValue >= c.minCount)) {
                    binMaxVal = binValue;
                    binMaxId = i;
                } else if (binValue < binMaxVal)
                    break;
                if ((last > 0) && (binValue == 0)) {
                    binMaxId = -1;  // :84 return false
                    break;
                }
            }
            if (!verdict && binMaxId >= 0) verdict = MLD_REGION_FLAG_HIST_FOUND;
            s_hist[0] = verdict;
            s_hist[1] = binMaxId;
        }
        __syncthreads();
        if (collect) from_list = true, n_list = cand;
        if (do_rad) {
            prefix = (prefix << 8) | (unsigned long long)s_digit;
            rank = s_rank;
            cand = s_cand;
        }
        if (do_hist) {
            flags |= s_hist[0];
            if (s_hist[0] & MLD_REGION_FLAG_HIST_FOUND) {
                lower = (double)s_hist[1] * c.binW - 0.0 * c.binW;   // :99
                higher = (double)s_hist[1] * c.binW + 1.0 * c.binW;  // :100
            }
        }
        if (do_seg) n_seg = s_seg;
        rad[tid] = 0;
        __syncthreads();
    }
    if (tid == 0) {
        rec->n_points = n, rec->n_ground = n_ground, rec->n_seg = n_seg, rec->flags = flags, rec->nearest_orig = orig;
        rec->clip[0] = cx0, rec->clip[1] = cy0, rec->clip[2] = cx1, rec->clip[3] = cy1;
        rec->pad_ = 0;
        rec->z_min = z_min, rec->z_max = z_max;
        rec->z_median = passes ? __longlong_as_double((long long)prefix) : z_min;
        rec->hist_lower = lower, rec->hist_higher = higher;
    }
}

char g_error[512] = "";  // refusals without an object: mld_region_depths_last_error(NULL)

}  // namespace

struct mld_region_depths : mld_batch::Object {
    int n_seq = 0;
    int64_t max_boxes = 0;
    RgCalib calib{};
    mld_batch::DescRing<RgSeq> ring;
};

extern "C" {

mld_region_depths* mld_region_depths_create(mld_ctx* ctx, int n_seq, int64_t max_boxes, const mld_params* params,
                                            const mld_camera* camera, int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first, then params and camera; the context last, and nothing of it is used before)
        if (n_seq < 1 || n_seq > 65536) return "mld_region_depths_create: n_seq must be in 1 .. 65536";
        if (max_boxes < 1) return "mld_region_depths_create: max_boxes must be at least 1";
        if (!params) return "mld_region_depths_create: null params";
        if (!camera) return "mld_region_depths_create: null camera";
        return nullptr;
    };
    const char* bad = refusal();
    const char* why = nullptr;
    int code = MLD_ERR_INVALID_ARG;
    if (!bad) {
        const double bw = params->histogram_segmentation_bin_witdh;
        if (!std::isfinite(bw) || !(bw > 0.0)) {
            why = "histogram_segmentation_bin_witdh must be finite and > 0";
        } else if (camera->width < 1 || camera->height < 1) {
            why = "bad image size";
        } else if (camera->width > 65535 || camera->height > 65535 || (int64_t)camera->width * camera->height > (int64_t)1 << 30) {
            why = "image larger than 65535 pixels on a side or 2^30 pixels in all";
            code = MLD_ERR_CAPACITY;
        } else if (max_boxes > kMaxGrid / n_seq) {
            why = "n_seq sequences of max_boxes boxes need more than 2^31 - 1 blocks";
            code = MLD_ERR_CAPACITY;
        }
        if (!why && !ctx) bad = "mld_region_depths_create: null context";
    }
    auto init = [&](mld_region_depths* rd) -> int {
        rd->n_seq = n_seq;
        rd->max_boxes = max_boxes;
        rd->calib.binW = params->histogram_segmentation_bin_witdh;
        rd->calib.minCount = params->histogram_segmentation_min_pointcount;
        rd->calib.W = camera->width;
        rd->calib.H = camera->height;
        rd->calib.listCap = kListCap;
#ifdef MLD_AB_SWITCHES
        if (const char* e = std::getenv("MLD_REGION_LIST_CAPACITY")) {
            const long v = std::strtol(e, nullptr, 10);
            rd->calib.listCap = (int)(v < 0 ? 0 : (v > kListCap ? kListCap : v));
        }
#endif
        return rd->ring.allocate(rd, n_seq);
    };
    return mld_batch::create_object<mld_region_depths>(g_error, "mld_region_depths_create", bad, ctx, status_out, init,
                                                       why ? code : MLD_OK, why);
}

void mld_region_depths_destroy(mld_region_depths* rd) { mld_batch::destroy_object(rd); }

const char* mld_region_depths_last_error(const mld_region_depths* rd) { return rd ? rd->err.c_str() : g_error; }

int mld_region_depths_collect_device(mld_region_depths* rd, const int32_t* const* map, const int32_t* const* index,
                                     const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                     const uint32_t* const* mask_dev, const int32_t* const* boxes, const int64_t* n_boxes,
                                     mld_region_depth* const* record_out) {
    const char* fn = "mld_region_depths_collect_device";
    if (!rd) return no_object(g_error, fn, "rd");
    auto refuse = [&](int code, const char* text) { return fail(rd, code, (std::string(fn) + ": " + text).c_str()); };
#define RG_REFUSE(text) return refuse(MLD_ERR_INVALID_ARG, text)
    if (!map) RG_REFUSE("null table map");
    if (!index) RG_REFUSE("null table index");
    if (!index_len) RG_REFUSE("null table index_len");
    if (!cam) RG_REFUSE("null table cam");
    if (!n_points) RG_REFUSE("null table n_points");
    if (!boxes) RG_REFUSE("null table boxes");
    if (!n_boxes) RG_REFUSE("null table n_boxes");
    if (!record_out) RG_REFUSE("null table record_out");
    const int S = rd->n_seq;
    int64_t per_seq = 0;
    for (int s = 0; s < S; s++) {
        if (index_len[s] < 0) RG_REFUSE("negative index_len");
        if (n_points[s] < 0) RG_REFUSE("negative n_points");
        if (n_boxes[s] < 0) RG_REFUSE("negative n_boxes");
        if (n_boxes[s] > rd->max_boxes) RG_REFUSE("n_boxes exceeds max_boxes");
        if (n_points[s] > kMaxPoints || index_len[s] > kMaxPoints) return refuse(MLD_ERR_CAPACITY, "n_points or index_len exceeds 8 388 607");
        if (!map[s]) RG_REFUSE("null array map");
        if (index_len[s] > 0 && !index[s]) RG_REFUSE("null array index of a sequence with index_len > 0");
        if (n_points[s] > 0 && !cam[s]) RG_REFUSE("null array cam of a sequence with n_points > 0");
        if (n_boxes[s] > 0 && !boxes[s]) RG_REFUSE("null array boxes of a sequence with n_boxes > 0");
        if (n_boxes[s] > 0 && !record_out[s]) RG_REFUSE("null array record_out of a sequence with n_boxes > 0");
        if (misaligned(map[s], 3u)) RG_REFUSE("map must be 4-byte aligned");
        if (misaligned(index[s], 3u)) RG_REFUSE("index must be 4-byte aligned");
        if (misaligned(cam[s], 7u)) RG_REFUSE("cam must be 8-byte aligned");
        if (mask_dev && misaligned(mask_dev[s], 3u)) RG_REFUSE("mask_dev must be 4-byte aligned");
        if (misaligned(boxes[s], 3u)) RG_REFUSE("boxes must be 4-byte aligned");
        if (misaligned(record_out[s], 7u)) RG_REFUSE("record_out must be 8-byte aligned");
        per_seq = n_boxes[s] > per_seq ? n_boxes[s] : per_seq;
    }
#undef RG_REFUSE
    if (per_seq == 0) return MLD_OK;  // (no box, no record: nothing to launch)
    for (int s = 0; s < S; s++) {
        RgSeq& q = rd->ring.stage[(size_t)s];
        q = RgSeq{};
        q.map = map[s];
        q.index = index[s];
        q.cam = cam[s];
        q.mask = mask_dev ? mask_dev[s] : nullptr;
        q.boxes = boxes[s];
        q.record = record_out[s];
        q.index_len = (int32_t)index_len[s];
        q.n_points = (int32_t)n_points[s];
        q.n_boxes = (int32_t)n_boxes[s];
    }
    MLD_HIP(rd, hipSetDevice(rd->device));
    const int rc = rd->ring.upload(rd);
    if (rc) return rc;
    hipLaunchKernelGGL(k_region_depths, dim3((unsigned)((int64_t)S * per_seq)), dim3(kBlock), 0, rd->stream, rd->ring.d_desc.get(), rd->calib,
                       (int)per_seq);
    MLD_HIP(rd, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
