// mld_depth_images.hip — dense depth images for a batch of sequences in one call (include/mld.h, "mld_depth_images"): the
// full per-feature path of DepthEstimator::CalculateDepth (DepthEstimator.cpp:491-600) at
// EVERY pixel of a grid over the camera image - narrow window, histogram segmentation, max-spanning triangle, planarity,
// viewing ray, Hyperplane::Through, thresholds, and the road fallback with its M-estimator fit.  The inputs are the arrays
// mld_projected_clouds_export_device writes (pixel map, _pointIndex, camera-frame cloud) and, optionally, the plane
// mld_semantic_planes / mld_ransac_planes leave on the device.  No frame slot is involved, nothing is allocated per call
// and nothing comes back to the host.
//
// Four launches: the descriptor upload and
//   k_depth_image_lane    ONE LANE PER GRID PIXEL.  A block of 256 threads takes a tile of kTileW x kTileH grid pixels;
//                         wavefront w takes the rows w * kRowsPerWave .. + kRowsPerWave - 1 of the tile, 64 pixels at a time.
//                         The cells the tile's windows reach (tile + halo of the wide window) are staged in LDS once, in one
//                         coalesced pass that also looks up and validates the point index of every OCCUPIED cell: a staged
//                         cell is the original index of its point, -1 (empty) or -2 (a value outside the arrays).  A tile
//                         whose region has more than kStageCells cells (large steps) reads the map directly instead.  A
//                         lane counts its narrow window from those cells: fewer than radiusSearch_count_min is type 2 and
//                         costs no list.  Otherwise the lane keeps up to kCap original indices in its LDS column and walks
//                         them in the reference's SERIAL order: histogram, triangle search, tail; then the wide window,
//                         the far test, the mask bits and the M-estimator fit, again serially.  A pixel whose narrow list or
//                         whose list of road inliers exceeds kCap writes nothing: its bit goes into the wavefront's overflow
//                         word.
//   k_depth_image_coop    one wavefront per wavefront of the lane kernel: for every bit of its overflow words, the same pixel
//                         WAVE-COOPERATIVELY, with lists of up to kMaxCells entries in LDS (the route of k_feature_trace).
//   k_depth_image_finish  per sequence: the record from the per-wavefront partial counts.
// The only ordering between blocks is the boundary between two launches: no atomics, no flags, no fences, no queue.  An
// overflow word and a row of partial counts have one writer per launch.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, V3, the wavefront helpers and the
// size limits: ../batch/mld_batch_device.h).  That path's arithmetic is restated, operation for operation, ONCE for the
// batch units, in ../batch/mld_depth_path.h: the cooperative route's stages behind the window scan (hist_segment,
// max_spanning_triangle, list_minmax_z), the tail both routes end in (finish_main with plane_through, viewing_ray,
// intersect, the thresholds), the window rule, the far test, and the calibration with Tinv and Kinv formed as mld_create
// forms them.  What stands here exists once - the lane route's serial walk over a lane's own list, the cell staging, the QR
// of the M-estimator and the one-sided Jacobi on its R, the counting - but for the cooperative route's gather_window, kept
// beside the header's for its code (see there).  This unit is compiled without contraction like the rest of the library.
// Main-path depths are bit for bit the reference's; road depths agree to the project's road tolerance (the sums of the fit
// are taken about the list's first point, not about the camera's origin: LAB.md 6.24).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"
#include "../batch/mld_depth_path.h"
#include "../../../include/mld.h"

namespace {

using namespace mld_batch;

constexpr int kBlock = 256;            // threads of the lane kernel and of the finish kernel
constexpr int kWaves = kBlock / kWave;
constexpr int kTileW = kWave;          // grid columns of a tile: a lane per column
constexpr int kRowsPerWave = 4;        // grid rows a wavefront of the lane kernel takes, one after the other
constexpr int kTileH = kWaves * kRowsPerWave;  // grid rows of a tile
constexpr int kCap = 32;               // entries of a lane's list (narrow neighbours; road inliers): 4 B x 256 lanes each
constexpr int kStageCells = 4096;      // cells of a tile's region that LDS holds (C0 at step 1: 84 x 31 = 2604)
constexpr int kPartInts = 32;          // a row of partial counts: counts[21], n_depth, n_cooperative, bad input, 8 unused
constexpr int kPartDepth = MLD_RESULT_TYPE_COUNT, kPartCoop = kPartDepth + 1, kPartBad = kPartDepth + 2;
constexpr int kOrigBits = 23;          // an original index fits (kMaxPoints = 2^23 - 1); the histogram's relative bin above
constexpr int kOrigMask = (1 << kOrigBits) - 1;
constexpr int kRelMax = 255;           // relative bins at and beyond it are never looked at (see lane_hist)
constexpr int64_t kMaxGrid = 2147483647;

static_assert(MLD_RESULT_TYPE_COUNT + 3 <= kPartInts, "a row of partial counts holds the record's sums");
static_assert(kMaxPoints <= kOrigMask, "an original index and a relative bin share an int32");
static_assert(sizeof(mld_depth_image_record) == 200, "200 bytes per record (include/mld.h)");
static_assert(offsetof(mld_depth_image_record, n_pixels) == 168 && offsetof(mld_depth_image_record, n_depth) == 176 &&
                  offsetof(mld_depth_image_record, n_cooperative) == 184 && offsetof(mld_depth_image_record, flags) == 192,
              "field offsets of the record (include/mld.h)");

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct DiSeq {
    const int32_t* map;    // W * H: visible index or -1
    const int32_t* index;  // index_len: original index of a visible point
    const double* cam;     // 3 x n_points
    const uint32_t* mask;  // ceil(n_points / 32) words; read only with has_plane
    double* depth;         // grid_w * grid_h each, or null
    float* depth32;
    uint8_t* type;
    double prior_n[3];     // M-estimator prior (DepthEstimator.cpp:286-292): normalize(a, b, c), d
    double prior_off;
    float coeffs[4];
    int32_t index_len;
    int32_t n_points;
    int32_t has_plane;
    int32_t pad_;
};
static_assert(sizeof(DiSeq) == 120, "120 bytes per sequence (include/mld.h, DESIGN.md)");

// What a call asks besides the descriptors.
struct DiCall {
    mld_depth_image_record* record;  // n_seq records
    int32_t x0, y0, step_x, step_y, grid_w, grid_h;
    int32_t tiles_x, tiles_y;
    int32_t force_coop;  // every pixel that clears the neighbour test takes the cooperative route (the A/B library only)
};

// Left singular vector of the smallest singular value of M = [sqrt(w_i) (p_i - c)] from the R of the thin QR of M^T
// (M M^T = R^T R): one-sided (Hestenes) Jacobi on the three rows of R^T, as the reference's JacobiSVD of M is restated on
// the rows of M itself (PlaneEstimationMEstimator.cpp:49).  R = r11 r12 r13 r22 r23 r33.
__device__ inline V3 normal_from_R(const double R[6]) {
    double B[3][3] = {{R[0], 0.0, 0.0}, {R[1], R[3], 0.0}, {R[2], R[4], R[5]}};
    double U[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double app = B[p][0] * B[p][0] + B[p][1] * B[p][1] + B[p][2] * B[p][2];
                const double aqq = B[q][0] * B[q][0] + B[q][1] * B[q][1] + B[q][2] * B[q][2];
                const double apq = B[p][0] * B[q][0] + B[p][1] * B[q][1] + B[p][2] * B[q][2];
                if (!(fabs(apq) > 1e-15 * sqrt(app * aqq)) || apq == 0.0) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double a = B[p][k], b = B[q][k];
                    B[p][k] = cs * a - sn * b;
                    B[q][k] = sn * a + cs * b;
                    const double ua = U[k][p], ub = U[k][q];
                    U[k][p] = cs * ua - sn * ub;
                    U[k][q] = sn * ua + cs * ub;
                }
            }
        if (!rotated) break;
    }
    double nrm[3];
#pragma unroll
    for (int r = 0; r < 3; r++) nrm[r] = B[r][0] * B[r][0] + B[r][1] * B[r][1] + B[r][2] * B[r][2];
    int m = 0;
    if (nrm[1] < nrm[0]) m = 1;
    if (nrm[2] < (m == 1 ? nrm[1] : nrm[0])) m = 2;
    V3 n0;
    n0.x = (m == 0) ? U[0][0] : ((m == 1) ? U[0][1] : U[0][2]);
    n0.y = (m == 0) ? U[1][0] : ((m == 1) ? U[1][1] : U[1][2]);
    n0.z = (m == 0) ? U[2][0] : ((m == 1) ? U[2][1] : U[2][2]);
    return n0;
}

// The tail of RoadDepthEstimatorMEstimator::CalculateDepth (:28-74) from the weighted centre and the R of the fit on.
__device__ __forceinline__ void finish_road(const DepthCalib& c, double u, double v, V3 center, const double R[6], double mn, double mx,
                                            int& out_type, double& out_depth) {
    const V3 dir = viewing_ray(c, u, v);
    const V3 support = {0, 0, 0};
    V3 n0 = normal_from_R(R);
    if (isnan(center.x) || isnan(center.y) || isnan(center.z)) {
        const double qn = __builtin_nan("");
        n0 = {qn, qn, qn};
    }
    Plane pl;
    pl.n = vnormalized(n0);
    pl.offset = -vdot(pl.n, center);
    double depth = -1.0;
    intersect(c, false, pl, dir, support, depth);  // n0 = direction, n1 = support (swapped, as the reference)
    int type = MLD_SuccessRoad;
    const int t = apply_thresholds(c, mn, mx, depth);
    if (t) type = t;
    out_type = type;
    out_depth = (type == MLD_SuccessRoad) ? depth : -1.0;
}

// A cell of the map as the path sees it: the original index of its point, -1 (empty) or -2 (a map value or an index value
// outside the arrays: counts as empty and sets the bad-input flag of whoever meets it).
__device__ __forceinline__ int classify_cell(const DiSeq& q, int m) {
    if (m == -1) return -1;
    if (m < 0 || m >= q.index_len) return -2;
    const int orig = as_global(q.index)[m];
    if (orig < 0 || orig >= q.n_points) return -2;
    return orig;
}

// The cells a tile of the lane kernel reads: staged in LDS (region rx0 .. rx0 + tw - 1, ry0 .. ry0 + th - 1) or the map.
struct Cells {
    const int32_t* lds;
    int rx0, ry0, tw, th;
    bool staged;
};
__device__ __forceinline__ int cell_at(const Cells& t, const DepthCalib& c, const DiSeq& q, int x, int y) {
    if (t.staged) {
        const int cx = x - t.rx0, cy = y - t.ry0;
        if ((unsigned)cx >= (unsigned)t.tw || (unsigned)cy >= (unsigned)t.th) return -1;  // (never: the region holds the windows)
        return t.lds[cy * t.tw + cx];
    }
    return classify_cell(q, as_global(q.map)[(size_t)x + (size_t)y * (size_t)c.W]);
}

__device__ __forceinline__ V3 cam_point(const DiSeq& q, int orig) {
    const MLD_BATCH_GLOBAL double* p = as_global(q.cam) + 3 * (size_t)orig;
    return {p[0], p[1], p[2]};
}
__device__ __forceinline__ double cam_z(const DiSeq& q, int orig) { return as_global(q.cam)[3 * (size_t)orig + 2]; }

// PlaneEstimationMEstimator.cpp:32: the weight of a point, 1 / absDistance to the prior
__device__ __forceinline__ double prior_weight(const DiSeq& q, V3 p) {
    const V3 pn = {q.prior_n[0], q.prior_n[1], q.prior_n[2]};
    return 1 / fabs(vdot(pn, p) + q.prior_off);
}

// ---------------------------------------------------------------------------------------------------------------------
// The lane route: everything below runs per lane on the lane's own list, lst[i * kBlock] = entry i (a column of LDS), in
// the reference's serial order.
// ---------------------------------------------------------------------------------------------------------------------

// PointHistogram::FilterPointsMinDistBlob (HistogramPointDepth.cpp:15-123, Histogram.cpp:14-49) on the k list entries: the
// points of the first local-maximum bin, compacted in place.  Returns their count or -1.  The bins ride in the entries'
// upper bits, relative to the first non-empty bin and saturated at kRelMax: the scan of :70-85 starts at a non-empty bin
// and leaves at the first empty one, so it looks at no more than k <= kCap consecutive bins.
__device__ __forceinline__ int lane_hist(const DepthCalib& c, const DiSeq& q, int* lst, int k) {
    int md = 0;  // :36-41: the largest ceil(depth) above 0
    for (int i = 0; i < k; i++) {
        double d = cam_z(q, lst[i * kBlock]);
        d = (999. < d) ? 999. : d;  // DepthEstimator.cpp:743
        if (d > (double)md) md = (int)ceil(d);
    }
    const int binCount = (int)((double)md / c.binW + 1.0);  // :43
    if (binCount <= 1) return -1;                           // :53
    const double lim = (double)binCount - 1.;
    int bmin = kNone;
    for (int i = 0; i < k; i++) {
        double d = cam_z(q, lst[i * kBlock]);
        d = (999. < d) ? 999. : d;
        const double value = (1e10 < d) ? 1e10 : d;  // Histogram.cpp:29
        const double qd = fabs(value / c.binW);
        const int bi = (int)((lim < qd) ? lim : qd);  // Histogram.cpp:30
        bmin = min(bmin, bi);
    }
    for (int i = 0; i < k; i++) {
        const int orig = lst[i * kBlock];
        double d = cam_z(q, orig);
        d = (999. < d) ? 999. : d;
        const double value = (1e10 < d) ? 1e10 : d;
        const double qd = fabs(value / c.binW);
        const int bi = (int)((lim < qd) ? lim : qd);
        lst[i * kBlock] = orig | (min(bi - bmin, kRelMax) << kOrigBits);
    }
    // HistogramPointDepth.cpp:70-85, started at the first non-empty bin (the empty bins ahead of it change nothing)
    int binMaxId = -1, binMaxVal = -1, binValue = 0;
    bool none = false;
    for (int i = bmin; i < binCount; i++) {
        const int last = binValue, rel = i - bmin;
        int cnt = 0;
        if (rel < kRelMax)
            for (int e = 0; e < k; e++) cnt += (((unsigned)lst[e * kBlock] >> kOrigBits) == (unsigned)rel) ? 1 : 0;
        binValue = cnt;
        if ((binValue > binMaxVal) && (binValue >= c.minCount)) {
            binMaxVal = binValue;
            binMaxId = i;
        } else if (binValue < binMaxVal)
            break;
        if ((last > 0) && (binValue == 0)) {
            none = true;
            break;
        }
    }
    int kk = -1;
    if (!none && binMaxId >= 0) {                                         // :95
        const double lower = (double)binMaxId * c.binW - 0.0 * c.binW;    // :99
        const double higher = (double)binMaxId * c.binW + 1.0 * c.binW;   // :100
        kk = 0;
        for (int i = 0; i < k; i++) {  // :115-120
            const int orig = lst[i * kBlock] & kOrigMask;
            const double z = cam_z(q, orig);
            const double d = (999. < z) ? 999. : z;
            if ((d >= lower) && (d < higher)) lst[(kk++) * kBlock] = orig;  // (kk <= i)
        }
    }
    return kk;  // (-1: the entries keep their bins; the road stage writes the list anew)
}

// PlaneEstimationCalcMaxSpanningTriangle::CalculatePlaneCorners (:37-100) with _distTreshold = 0 on the n list entries, in
// the serial loops' order: strict '>' keeps the first maximal pair and the first maximal third corner.
__device__ __forceinline__ bool lane_triangle(const DiSeq& q, const int* lst, int n, V3& c1, V3& c2, V3& c3) {
    if (n < 3) return false;
    double bd = -1.0;
    int bi = -1, bj = -1;
    for (int i = 0; i < n - 1; i++) {
        const V3 pi = cam_point(q, lst[i * kBlock]);
        for (int j = i + 1; j < n; j++) {
            const double d = vsqnorm(vsub(pi, cam_point(q, lst[j * kBlock])));
            if (d > bd) {
                bd = d;
                bi = i;
                bj = j;
            }
        }
    }
    if (bi < 0 || bd <= 0.0) return false;  // :65
    const V3 pa = cam_point(q, lst[bi * kBlock]), pb = cam_point(q, lst[bj * kBlock]);
    double b2 = -1.0;
    int bk = -1;
    V3 pk3 = pa;
    for (int kx = 0; kx < n - 1; kx++) {  // :71 the last point is never considered
        if (kx == bi || kx == bj) continue;
        const V3 pk = cam_point(q, lst[kx * kBlock]);
        const double d1 = vsqnorm(vsub(pk, pa));
        if (d1 <= 0.0) continue;
        const double d2 = vsqnorm(vsub(pk, pb));
        if (d2 <= 0.0) continue;
        const double d = d1 + d2;
        if (d > b2) {
            b2 = d;
            bk = kx;
            pk3 = pk;
        }
    }
    if (bk < 0) return false;
    c1 = pa;
    c2 = pb;
    c3 = pk3;
    return true;
}

// PlaneEstimationMEstimator::EstimatePlane (:18-55) up to the decomposition, on the n list entries: the weighted centre -
// its sums taken about the list's first point - and the R of the thin QR of M^T, M = [sqrt(w_i) (p_i - c)], by modified
// Gram-Schmidt; the rows are recomputed in every pass instead of being kept.
__device__ __forceinline__ void lane_road_qr(const DiSeq& q, const int* lst, int n, V3& center, double R[6], double& mn, double& mx) {
    const V3 p0 = cam_point(q, lst[0]);
    double sw = 0, sx = 0, sy = 0, sz = 0;
    mn = kDblMax, mx = -kDblMax;
    for (int i = 0; i < n; i++) {
        const V3 p = cam_point(q, lst[i * kBlock]);
        const double w = prior_weight(q, p);
        sw += w;
        sx += w * (p.x - p0.x);
        sy += w * (p.y - p0.y);
        sz += w * (p.z - p0.z);
        if (p.z < mn) mn = p.z;  // TresholdDepthLocal.cpp:23-29
        if (p.z > mx) mx = p.z;
    }
    const double cx = p0.x + sx / sw, cy = p0.y + sy / sw, cz = p0.z + sz / sw;
    center = {cx, cy, cz};
#define DI_ROW(i)                                             \
    const V3 p = cam_point(q, lst[(i) * kBlock]);             \
    const double ws = sqrt(prior_weight(q, p));               \
    const double ax = ws * (p.x - cx), ay = ws * (p.y - cy), az = ws * (p.z - cz)
    double t0 = 0;
    for (int i = 0; i < n; i++) {
        DI_ROW(i);
        (void)ay, (void)az;
        t0 += ax * ax;
    }
    const double r11 = sqrt(t0);
    const double i11 = r11 > 0.0 ? 1 / r11 : 0.0;  // (all points in one place: a zero column stays zero)
    double r12 = 0, r13 = 0;
    for (int i = 0; i < n; i++) {
        DI_ROW(i);
        const double q1 = ax * i11;
        r12 += q1 * ay;
        r13 += q1 * az;
    }
    t0 = 0;
    for (int i = 0; i < n; i++) {
        DI_ROW(i);
        (void)az;
        const double q1 = ax * i11;
        const double by = ay - r12 * q1;
        t0 += by * by;
    }
    const double r22 = sqrt(t0);
    const double i22 = r22 > 0.0 ? 1 / r22 : 0.0;
    double r23 = 0;
    for (int i = 0; i < n; i++) {
        DI_ROW(i);
        const double q1 = ax * i11;
        const double q2 = (ay - r12 * q1) * i22;
        r23 += q2 * (az - r13 * q1);
    }
    t0 = 0;
    for (int i = 0; i < n; i++) {
        DI_ROW(i);
        const double q1 = ax * i11;
        const double q2 = (ay - r12 * q1) * i22;
        const double bz = (az - r13 * q1) - r23 * q2;
        t0 += bz * bz;
    }
#undef DI_ROW
    R[0] = r11, R[1] = r12, R[2] = r13, R[3] = r22, R[4] = r23, R[5] = sqrt(t0);
}

// One grid pixel on one lane.  Returns false when the pixel leaves the lane route (nothing of it is final then).
__device__ __forceinline__ bool lane_pixel(const DepthCalib& c, const DiSeq& q, const DiCall& call, const Cells& cells, int* lst, int px, int py,
                                           int& out_type, double& out_depth, bool& bad) {
    const double u = (double)px, v = (double)py;
    int xl, xh, yl, yh;
    // ---- B2: the narrow window (DepthEstimator.cpp:509, scale 1.0 x 1.0) ----
    window_bounds(px, c.halfX1, c.W - 1, xl, xh);
    window_bounds(py, c.halfY1, c.H - 1, yl, yh);
    int k = 0;
    for (int y = yl; y <= yh; y++)
        for (int x = xl; x <= xh; x++) {
            const int o = cell_at(cells, c, q, x, y);
            if (o == -2) bad = true;
            if (o >= 0) {
                if (k < kCap) lst[k * kBlock] = o;
                k++;
            }
        }
    out_depth = -1.0;
    if ((unsigned)k < c.countMin) {  // :680, compared as unsigned
        out_type = MLD_RadiusSearchInsufficientPoints;
        return true;
    }
    if (k > kCap || call.force_coop) return false;
    // ---- B3: CalculateDepthSegmentation (:726-780) ----
    int type = MLD_Unspecified;
    double depth = -1.0;
    int ks = k;
    if (c.useHist) ks = lane_hist(c, q, lst, k);
    if (ks < 0) {
        type = MLD_HistogramNoLocalMax;
    } else {
        // ---- B5: the corners (:915-926) ----
        bool ok = true;
        V3 c1 = {0, 0, 0}, c2 = c1, c3 = c1;
        if (c.useTriMax) {
            ok = lane_triangle(q, lst, ks, c1, c2, c3);
            if (!ok) type = MLD_TriangleNotPlanarInsufficientPoints;
        } else if (ks < 3) {
            ok = false;
            type = MLD_HistogramNoLocalMax;  // :920-921
        } else {
            c1 = cam_point(q, lst[0]), c2 = cam_point(q, lst[kBlock]), c3 = cam_point(q, lst[2 * kBlock]);
        }
        if (ok) {
            double mn = kDblMax, mx = -kDblMax;  // TresholdDepthLocal.cpp:23-29
            for (int i = 0; i < ks; i++) {
                const double z = cam_z(q, lst[i * kBlock]);
                if (z < mn) mn = z;
                if (z > mx) mx = z;
            }
            type = finish_main(c, u, v, c1, c2, c3, mn, mx, nullptr, depth);  // ---- B6 ----
        }
    }
    // ---- the road fallback (:578-597) ----
    if (c.useRoad && q.has_plane && type != MLD_Success) {
        window_bounds(px, c.halfX2, c.W - 1, xl, xh);
        window_bounds(py, c.halfY2, c.H - 1, yl, yh);
        int k2 = 0, kk = 0;
        bool anyFar = false;
        for (int y = yl; y <= yh; y++)
            for (int x = xl; x <= xh; x++) {
                const int o = cell_at(cells, c, q, x, y);
                if (o == -2) bad = true;
                if (o >= 0) {
                    k2++;
                    if (!anyFar) {  // (the reference leaves at the first far neighbour: the rest only counts)
                        if (far_from_plane(c.Tinv, q.coeffs, c.roadDistThr, cam_point(q, o))) {
                            anyFar = true;
                        } else if (mask_bit(q.mask, o)) {
                            if (kk < kCap) lst[kk * kBlock] = o;
                            kk++;
                        }
                    }
                }
            }
        if ((unsigned)k2 < c.countMin) {  // :585-586
            type = MLD_RadiusSearchInsufficientPoints;
            depth = -1.0;
        } else if (!anyFar && kk >= 3) {  // :591, :827-829: else the main path's result stays
            if (kk > kCap) return false;
            V3 center;
            double R[6], mn, mx;
            lane_road_qr(q, lst, kk, center, R, mn, mx);
            finish_road(c, u, v, center, R, mn, mx, type, depth);
        }
    }
    out_type = type;
    out_depth = depth;
    return true;
}

__device__ __forceinline__ void store_pixel(const DiSeq& q, size_t at, int type, double depth) {
    if (q.type) as_global(q.type)[at] = (uint8_t)type;
    if (q.depth) as_global(q.depth)[at] = depth;
    if (q.depth32) as_global(q.depth32)[at] = (float)depth;
}

// Into lane t of `cnt`: how many of the wavefront's pixels (those with `final`) have type t; lane kPartDepth: how many have
// a depth.
__device__ __forceinline__ void count_types(int& cnt, int lane, bool final, int type, double depth) {
#pragma unroll
    for (int t = 0; t < MLD_RESULT_TYPE_COUNT; t++) {
        const int n = (int)__popcll(__ballot(final && type == t));
        if (lane == t) cnt += n;
    }
    const int n = (int)__popcll(__ballot(final && depth >= 0));
    if (lane == kPartDepth) cnt += n;
}

// Grid: n_seq * tiles_x * tiles_y blocks.  over: kRowsPerWave words per wavefront; part: kPartInts ints per wavefront.
__global__ __launch_bounds__(kBlock) void k_depth_image_lane(const DiSeq* __restrict__ desc, DepthCalib c, DiCall call, unsigned long long* over,
                                                             int32_t* part) {
    __shared__ int32_t lists[kCap * kBlock];
    __shared__ int32_t staged[kStageCells];
    const int per_seq = call.tiles_x * call.tiles_y;
    const int s = (int)(blockIdx.x / (unsigned)per_seq), rem = (int)(blockIdx.x % (unsigned)per_seq);
    const int ty = rem / call.tiles_x, tx = rem - ty * call.tiles_x;
    const DiSeq q = desc[s];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    // the region of the image the tile's windows reach: the wide windows of its first and its last pixel, per axis
    const int gi0 = tx * kTileW, gj0 = ty * kTileH;
    const int gi1 = min(gi0 + kTileW, call.grid_w) - 1, gj1 = min(gj0 + kTileH, call.grid_h) - 1;
    Cells cells;
    int lo, hi;
    window_bounds(call.x0 + gi0 * call.step_x, c.halfX2, c.W - 1, cells.rx0, hi);
    window_bounds(call.x0 + gi1 * call.step_x, c.halfX2, c.W - 1, lo, hi);
    cells.tw = hi - cells.rx0 + 1;
    window_bounds(call.y0 + gj0 * call.step_y, c.halfY2, c.H - 1, cells.ry0, hi);
    window_bounds(call.y0 + gj1 * call.step_y, c.halfY2, c.H - 1, lo, hi);
    cells.th = hi - cells.ry0 + 1;
    cells.lds = staged;
    cells.staged = cells.tw >= 1 && cells.th >= 1 && (long long)cells.tw * (long long)cells.th <= (long long)kStageCells;
    if (cells.staged) {  // one coalesced pass over the region; the index is fetched for occupied cells only
        const int ncell = cells.tw * cells.th;
        for (int i = tid; i < ncell; i += kBlock) {
            const int r = i / cells.tw, col = i - r * cells.tw;
            staged[i] = classify_cell(q, as_global(q.map)[(size_t)(cells.rx0 + col) + (size_t)(cells.ry0 + r) * (size_t)c.W]);
        }
    }
    __syncthreads();
    int cnt = 0;
    bool bad = false;
    const size_t wave_id = (size_t)blockIdx.x * kWaves + (size_t)w;
    for (int rr = 0; rr < kRowsPerWave; rr++) {
        const int gi = gi0 + lane, gj = gj0 + w * kRowsPerWave + rr;
        const bool valid = gi < call.grid_w && gj < call.grid_h;
        int type = 0;
        double depth = -1.0;
        bool done = false;
        if (valid) {
            done = lane_pixel(c, q, call, cells, lists + tid, call.x0 + gi * call.step_x, call.y0 + gj * call.step_y, type, depth, bad);
            if (done) store_pixel(q, (size_t)gi + (size_t)gj * (size_t)call.grid_w, type, depth);
        }
        const unsigned long long ov = __ballot(valid && !done);
        if (lane == 0) as_global(over)[wave_id * kRowsPerWave + rr] = ov;
        count_types(cnt, lane, valid && done, type, depth);
        if (lane == kPartCoop) cnt += (int)__popcll(ov);
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == kPartBad) cnt = any_bad ? 1 : 0;
    if (lane < kPartInts) as_global(part)[wave_id * kPartInts + lane] = cnt;
}

// ---------------------------------------------------------------------------------------------------------------------
// The cooperative route: one wavefront per pixel, lists of up to c.cap entries in LDS (dynamic; 28 bytes per entry), worked
// on by the functions of the depth path's header.
// ---------------------------------------------------------------------------------------------------------------------
struct Lists : PointList {
    int32_t* aux;  // the histogram's bin of neighbour i; in the road stage its original index
};

// Window scan (NeighborFinderPixel.cpp:60-95) + 3-D gather (NeighborFinderBase.cpp:15-27): the neighbours in the
// reference's row-major scan order; their count (wave-uniform, <= c.cap because the window has at most that many cells).
// This unit's own copy of the depth path header's gather_window, on the staged cells' classification and integer pixels:
// through the shared one k_depth_image_coop grew by 39 instructions and the forced cooperative route measured slower than
// the band allows (profiles/depth_path_header.md).  A correction to either belongs in both.
__device__ __forceinline__ int gather_window(const DepthCalib& c, const DiSeq& q, int px, int py, double halfX, double halfY, const Lists& L,
                                             int lane, bool& bad) {
    int x0, x1, y0, y1;
    window_bounds(px, halfX, c.W - 1, x0, x1);
    window_bounds(py, halfY, c.H - 1, y0, y1);
    x0 = uniform(x0), x1 = uniform(x1), y0 = uniform(y0), y1 = uniform(y1);
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    if (nx <= 0 || ny <= 0) return 0;
    if (x0 < 0 || y0 < 0 || x1 >= c.W || y1 >= c.H) return 0;        // unreachable for a pixel of the image
    if ((long long)nx * (long long)ny > (long long)c.cap) return 0;  // unreachable: the object's bound on the window
    const int ncell = nx * ny;
    const MLD_BATCH_GLOBAL int32_t* map = as_global(q.map);
    const MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    int k = 0;
    bool badl = false;
    for (int base = 0; base < ncell; base += kWave) {
        const int cidx = base + lane;
        int o = -1;
        if (cidx < ncell) {
            const int r = cidx / nx, col = cidx - r * nx;
            o = classify_cell(q, map[(size_t)(x0 + col) + (size_t)(y0 + r) * (size_t)c.W]);
        }
        if (o == -2) badl = true;
        const bool has = o >= 0;
        const unsigned long long mk = __ballot(has);
        const int rank = k + prefix_count(mk);
        if (has && rank < c.cap) {
            L.x[rank] = cam[3 * (size_t)o];
            L.y[rank] = cam[3 * (size_t)o + 1];
            L.z[rank] = cam[3 * (size_t)o + 2];
            L.aux[rank] = o;
        }
        k += (int)__popcll(mk);
    }
    if (__ballot(badl) != 0ull) bad = true;
    k = uniform(k);
    return k < c.cap ? k : c.cap;
}

// lane_road_qr over the wavefront: the rows a_i = sqrt(w_i) (p_i - c) are written over the list (nothing reads it
// afterwards) and orthogonalised there.
__device__ __forceinline__ void road_qr(int n, const Lists& L, int lane, const DiSeq& q, V3& center, double R[6]) {
    const V3 p0 = list_point(L, 0);
    double sw = 0, sx = 0, sy = 0, sz = 0;
    for (int i = lane; i < n; i += kWave) {
        const V3 p = list_point(L, i);
        const double w = prior_weight(q, p);
        sw += w;
        sx += w * (p.x - p0.x);
        sy += w * (p.y - p0.y);
        sz += w * (p.z - p0.z);
    }
    sw = wave_sum(sw);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    sz = wave_sum(sz);
    const double cx = p0.x + sx / sw, cy = p0.y + sy / sw, cz = p0.z + sz / sw;
    center = {cx, cy, cz};
    __syncthreads();  // (every lane has read the first point)
    double t0 = 0;
    for (int i = lane; i < n; i += kWave) {
        const V3 p = list_point(L, i);
        const double ws = sqrt(prior_weight(q, p));
        const double ax = ws * (p.x - cx), ay = ws * (p.y - cy), az = ws * (p.z - cz);
        L.x[i] = ax;
        L.y[i] = ay;
        L.z[i] = az;
        t0 += ax * ax;
    }
    const double r11 = sqrt(wave_sum(t0));
    const double i11 = r11 > 0.0 ? 1 / r11 : 0.0;  // (all points in one place: a zero column stays zero)
    double t1 = 0, t2 = 0;
    for (int i = lane; i < n; i += kWave) {
        const double q1 = L.x[i] * i11;
        L.x[i] = q1;
        t1 += q1 * L.y[i];
        t2 += q1 * L.z[i];
    }
    const double r12 = wave_sum(t1), r13 = wave_sum(t2);
    t0 = 0;
    for (int i = lane; i < n; i += kWave) {
        const double q1 = L.x[i];
        const double ay = L.y[i] - r12 * q1;
        L.y[i] = ay;
        L.z[i] = L.z[i] - r13 * q1;
        t0 += ay * ay;
    }
    const double r22 = sqrt(wave_sum(t0));
    const double i22 = r22 > 0.0 ? 1 / r22 : 0.0;
    t1 = 0;
    for (int i = lane; i < n; i += kWave) {
        const double q2 = L.y[i] * i22;
        L.y[i] = q2;
        t1 += q2 * L.z[i];
    }
    const double r23 = wave_sum(t1);
    t0 = 0;
    for (int i = lane; i < n; i += kWave) {
        const double az = L.z[i] - r23 * L.y[i];
        t0 += az * az;
    }
    R[0] = r11, R[1] = r12, R[2] = r13, R[3] = r22, R[4] = r23, R[5] = sqrt(wave_sum(t0));
}

// One grid pixel on one wavefront; type and depth are wave-uniform.
__device__ __forceinline__ void coop_pixel(const DepthCalib& c, const DiSeq& q, const Lists& L, int lane, int px, int py, int& out_type,
                                           double& out_depth, bool& bad) {
    const double u = (double)px, v = (double)py;
    int type = MLD_Unspecified;
    double depth = -1.0;
    // ---- B2: the narrow window ----
    const int n_nb = gather_window(c, q, px, py, c.halfX1, c.halfY1, L, lane, bad);
    __syncthreads();
    if ((unsigned)n_nb < c.countMin) {  // :680, compared as unsigned
        out_type = MLD_RadiusSearchInsufficientPoints;
        out_depth = -1.0;
        return;
    }
    // ---- B3 ----
    int ks = n_nb;
    double lower, higher;  // (the chosen bin's borders: the trace's business)
    if (c.useHist) ks = hist_segment(c, n_nb, L, L.aux, lane, lower, higher, [](int, int) {});
    __syncthreads();
    if (ks < 0) {
        type = MLD_HistogramNoLocalMax;
    } else {
        // ---- B5 ----
        bool ok = true;
        int ci = 0, cj = 1, ck = 2;
        if (c.useTriMax) {
            ok = max_spanning_triangle(ks, L, lane, ci, cj, ck);
            if (!ok) type = MLD_TriangleNotPlanarInsufficientPoints;
        } else if (ks < 3) {
            ok = false;
            type = MLD_HistogramNoLocalMax;  // :920-921
        }
        if (ok) {
            double mn, mx;
            list_minmax_z(ks, L, lane, mn, mx);
            type = finish_main(c, u, v, list_point(L, ci), list_point(L, cj), list_point(L, ck), mn, mx, nullptr, depth);  // ---- B6 ----
        }
    }
    __syncthreads();  // (the lists are rewritten from here)
    // ---- the road fallback (:578-597) ----
    if (c.useRoad && q.has_plane && type != MLD_Success) {
        const int n_road = gather_window(c, q, px, py, c.halfX2, c.halfY2, L, lane, bad);
        __syncthreads();
        if ((unsigned)n_road < c.countMin) {  // :585-586
            type = MLD_RadiusSearchInsufficientPoints;
            depth = -1.0;
        } else {
            // CalculateDepthSegmentationPlane (:782-900): the inliers compacted in place
            bool anyFar = false;
            int kk = 0;
            for (int b = 0; b < n_road; b += kWave) {
                const int i = b + lane;
                bool far = false, inl = false;
                V3 p = {0, 0, 0};
                if (i < n_road) {
                    p = list_point(L, i);
                    far = far_from_plane(c.Tinv, q.coeffs, c.roadDistThr, p);
                    inl = mask_bit(q.mask, L.aux[i]);
                }
                anyFar = anyFar || (__ballot(far) != 0ull);
                const unsigned long long m = __ballot(inl);
                const int rank = kk + prefix_count(m);  // (<= i)
                if (inl) {
                    L.x[rank] = p.x;
                    L.y[rank] = p.y;
                    L.z[rank] = p.z;
                }
                kk += (int)__popcll(m);
            }
            kk = uniform(kk);
            __syncthreads();
            if (!anyFar && kk >= 3) {  // :591, :827-829: else the main path's result stays
                double mn, mx, R[6];
                V3 center;
                list_minmax_z(kk, L, lane, mn, mx);
                __syncthreads();
                road_qr(kk, L, lane, q, center, R);
                finish_road(c, u, v, center, R, mn, mx, type, depth);
            }
        }
    }
    out_type = type;
    out_depth = depth;
}

// Grid: one block of one wavefront per wavefront of the lane kernel (n_seq * tiles * kWaves).
__global__ __launch_bounds__(kWave) void k_depth_image_coop(const DiSeq* __restrict__ desc, DepthCalib c, DiCall call, const unsigned long long* over,
                                                            int32_t* part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t wave_id = (size_t)blockIdx.x;
    const int lane = (int)threadIdx.x;
    unsigned long long words[kRowsPerWave];
    unsigned long long any = 0ull;
#pragma unroll
    for (int rr = 0; rr < kRowsPerWave; rr++) {
        words[rr] = as_global(over)[wave_id * kRowsPerWave + rr];
        any |= words[rr];
    }
    if (any == 0ull) return;  // (uniform)
    const int block = (int)(blockIdx.x / (unsigned)kWaves), w = (int)(blockIdx.x % (unsigned)kWaves);
    const int per_seq = call.tiles_x * call.tiles_y;
    const int s = block / per_seq, rem = block - s * per_seq;
    const int ty = rem / call.tiles_x, tx = rem - ty * call.tiles_x;
    const DiSeq q = desc[s];
    Lists L;
    L.x = reinterpret_cast<double*>(smem);
    L.y = L.x + c.cap;
    L.z = L.y + c.cap;
    L.aux = reinterpret_cast<int32_t*>(L.z + c.cap);
    int cnt = 0;
    bool bad = false;
#pragma unroll 1
    for (int rr = 0; rr < kRowsPerWave; rr++) {
        const int gj = ty * kTileH + w * kRowsPerWave + rr;
        for (unsigned long long m = words[rr]; m; m &= m - 1) {  // (uniform)
            const int gi = tx * kTileW + (__ffsll((long long)m) - 1);
            if (gi >= call.grid_w || gj >= call.grid_h) continue;  // (never: the lane kernel sets bits of valid pixels only)
            int type;
            double depth;
            coop_pixel(c, q, L, lane, call.x0 + gi * call.step_x, call.y0 + gj * call.step_y, type, depth, bad);
            __syncthreads();  // (the next pixel rewrites the lists)
            type = uniform(type);
            if (lane == 0) store_pixel(q, (size_t)gi + (size_t)gj * (size_t)call.grid_w, type, depth);
            if (lane == type) cnt += 1;
            if (lane == kPartDepth && depth >= 0) cnt += 1;
        }
    }
    if (lane == kPartBad) cnt = bad ? 1 : 0;
    // the wavefront's row of partial counts: the lane kernel wrote it, this block alone adds to it
    if (lane < kPartCoop || lane == kPartBad) {
        MLD_BATCH_GLOBAL int32_t* row = as_global(part) + wave_id * kPartInts;
        row[lane] = lane == kPartBad ? (row[lane] | cnt) : row[lane] + cnt;
    }
}

// Grid: n_seq blocks.  The record of a sequence from the rows of partial counts of its wavefronts.
__global__ __launch_bounds__(kBlock) void k_depth_image_finish(const DiSeq* __restrict__ desc, DiCall call, const int32_t* part) {
    constexpr int kStripes = kBlock / kPartInts;
    __shared__ long long sums[kStripes][kPartInts];
    const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int col = tid & (kPartInts - 1), stripe = tid / kPartInts;
    const long long rows = (long long)call.tiles_x * call.tiles_y * kWaves;
    const MLD_BATCH_GLOBAL int32_t* base = as_global(part) + (size_t)s * (size_t)rows * kPartInts;
    long long acc = 0;
    for (long long r = stripe; r < rows; r += kStripes) acc += base[(size_t)r * kPartInts + col];
    sums[stripe][col] = acc;
    __syncthreads();
    if (tid < kPartInts) {
        long long t = 0;
#pragma unroll
        for (int k = 0; k < kStripes; k++) t += sums[k][tid];
        sums[0][tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        MLD_BATCH_GLOBAL mld_depth_image_record* rec = as_global(call.record) + s;
        for (int t = 0; t < MLD_RESULT_TYPE_COUNT; t++) rec->counts[t] = sums[0][t];
        rec->n_pixels = (long long)call.grid_w * (long long)call.grid_h;
        rec->n_depth = sums[0][kPartDepth];
        rec->n_cooperative = sums[0][kPartCoop];
        rec->flags = (sums[0][kPartBad] ? MLD_DEPTH_IMAGE_FLAG_BAD_INPUT : 0) | (desc[s].has_plane ? MLD_DEPTH_IMAGE_FLAG_HAS_PLANE : 0);
        rec->pad_ = 0;
    }
}

char g_error[512] = "";  // refusals without an object: mld_depth_images_last_error(NULL)

int64_t tiles_of(int grid_w, int grid_h) { return (int64_t)((grid_w + kTileW - 1) / kTileW) * (int64_t)((grid_h + kTileH - 1) / kTileH); }

// What only this object refuses, then what mld_create refuses of a parameter set, a camera and a transform, with its texts.
int refuse_config(const mld_params& P, const mld_camera& cam, const double T[12], int n_seq, std::string& why) {
    if (P.do_use_PCA) {
        why = "do_use_PCA: the eigen-solve is a tolerance path, the depth image promises equality on the main path";
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    if (P.plane_estimator_use_triangle_maximation) {
        why = "plane_estimator_use_triangle_maximation: the triangle road estimator is a rare path, use the depth calls";
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
    if (code != MLD_OK) return code;
    if ((int64_t)n_seq * tiles_of(cam.width, cam.height) * kWaves > kMaxGrid) {
        why = "n_seq sequences of this image size need more than 2^31 - 1 blocks";
        return MLD_ERR_CAPACITY;
    }
    return MLD_OK;
}

}  // namespace

struct mld_depth_images : mld_batch::Object {
    int n_seq = 0;
    int force_coop = 0;
    DepthCalib calib{};
    size_t lds_bytes = 0;                  // of k_depth_image_coop
    int64_t max_tiles = 0;                 // tiles of the full grid of one sequence
    mld_batch::DeviceBuffer<unsigned long long> d_over;  // n_seq x max_tiles x kWaves x kRowsPerWave overflow words
    mld_batch::DeviceBuffer<int32_t> d_part;             // n_seq x max_tiles x kWaves x kPartInts partial counts
    mld_batch::DescRing<DiSeq> ring;
};

extern "C" {

mld_depth_images* mld_depth_images_create(mld_ctx* ctx, int n_seq, const mld_params* params, const mld_camera* camera,
                                          const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        if (n_seq < 1 || n_seq > 65536) return "mld_depth_images_create: n_seq must be in 1 .. 65536";
        if (!params) return "mld_depth_images_create: null params";
        if (!camera) return "mld_depth_images_create: null camera";
        if (!T_cam_lidar) return "mld_depth_images_create: null T_cam_lidar";
        return nullptr;
    };
    const char* bad = refusal();
    std::string why;
    int code = MLD_OK;
    if (!bad) {  // (what is refused with a status of its own; the context has not been looked at yet)
        code = refuse_config(*params, *camera, T_cam_lidar, n_seq, why);
        // (the last refusal: everything else was judged without it)
        if (code == MLD_OK && !ctx) bad = "mld_depth_images_create: null context";
    }
    auto init = [&](mld_depth_images* di) -> int {
        di->n_seq = n_seq;
        build_calib(di->calib, *params, *camera, T_cam_lidar);
#ifdef MLD_AB_SWITCHES
        const char* e = std::getenv("MLD_DEPTH_IMAGE_COOP");
        di->force_coop = (e && e[0] == '1') ? 1 : 0;
#endif
        di->lds_bytes = (size_t)di->calib.cap * 28;
        di->max_tiles = tiles_of(camera->width, camera->height);
        const size_t waves = (size_t)n_seq * (size_t)di->max_tiles * kWaves;
        int rc;
        if ((rc = di->d_over.allocate(di, waves * kRowsPerWave))) return rc;
        if ((rc = di->d_part.allocate(di, waves * kPartInts))) return rc;
        return di->ring.allocate(di, n_seq);
    };
    return mld_batch::create_object<mld_depth_images>(g_error, "mld_depth_images_create", bad, ctx, status_out, init, code,
                                                      why.c_str());
}

void mld_depth_images_destroy(mld_depth_images* di) { mld_batch::destroy_object(di); }

const char* mld_depth_images_last_error(const mld_depth_images* di) { return di ? di->err.c_str() : g_error; }

int mld_depth_images_render_device(mld_depth_images* di, const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                   const double* const* cam, const int64_t* n_points, const float* coeffs, const uint32_t* const* mask_dev,
                                   int x0, int y0, int step_x, int step_y, int grid_w, int grid_h, double* const* depth_out,
                                   float* const* depth32_out, uint8_t* const* type_out, mld_depth_image_record* record_out_dev) {
    const char* fn = "mld_depth_images_render_device";
    if (!di) return no_object(g_error, fn, "di");
    auto refuse = [&](int code, const char* text) { return fail(di, code, (std::string(fn) + ": " + text).c_str()); };
#define DI_REFUSE(text) return refuse(MLD_ERR_INVALID_ARG, text)
    if (!map) DI_REFUSE("null table map");
    if (!index) DI_REFUSE("null table index");
    if (!index_len) DI_REFUSE("null table index_len");
    if (!cam) DI_REFUSE("null table cam");
    if (!n_points) DI_REFUSE("null table n_points");
    if (!record_out_dev) DI_REFUSE("null array record_out_dev");
    if (misaligned(record_out_dev, 7u)) DI_REFUSE("record_out_dev must be 8-byte aligned");
    if ((coeffs != nullptr) != (mask_dev != nullptr)) DI_REFUSE("coeffs and mask_dev come together or not at all");
    const DepthCalib& c = di->calib;
    if (step_x < 1) DI_REFUSE("step_x must be >= 1");
    if (step_y < 1) DI_REFUSE("step_y must be >= 1");
    if (grid_w < 1) DI_REFUSE("grid_w must be >= 1");
    if (grid_h < 1) DI_REFUSE("grid_h must be >= 1");
    if (x0 < 0 || x0 >= c.W) DI_REFUSE("x0 lies outside the image");
    if (y0 < 0 || y0 >= c.H) DI_REFUSE("y0 lies outside the image");
    if ((int64_t)x0 + ((int64_t)grid_w - 1) * (int64_t)step_x > (int64_t)c.W - 1)
        DI_REFUSE("grid_w: the last column x0 + (grid_w - 1) * step_x lies outside the image");
    if ((int64_t)y0 + ((int64_t)grid_h - 1) * (int64_t)step_y > (int64_t)c.H - 1)
        DI_REFUSE("grid_h: the last row y0 + (grid_h - 1) * step_y lies outside the image");
    const int S = di->n_seq;
    for (int s = 0; s < S; s++) {
        if (index_len[s] < 0) DI_REFUSE("negative index_len");
        if (n_points[s] < 0) DI_REFUSE("negative n_points");
        if (n_points[s] > kMaxPoints || index_len[s] > kMaxPoints) return refuse(MLD_ERR_CAPACITY, "n_points or index_len exceeds 8 388 607");
        if (!map[s]) DI_REFUSE("null array map");
        if (index_len[s] > 0 && !index[s]) DI_REFUSE("null array index of a sequence with index_len > 0");
        if (n_points[s] > 0 && !cam[s]) DI_REFUSE("null array cam of a sequence with n_points > 0");
        if (misaligned(map[s], 3u)) DI_REFUSE("map must be 4-byte aligned");
        if (misaligned(index[s], 3u)) DI_REFUSE("index must be 4-byte aligned");
        if (misaligned(cam[s], 7u)) DI_REFUSE("cam must be 8-byte aligned");
        if (mask_dev && misaligned(mask_dev[s], 3u)) DI_REFUSE("mask_dev must be 4-byte aligned");
        if (depth_out && misaligned(depth_out[s], 7u)) DI_REFUSE("depth_out must be 8-byte aligned");
        if (depth32_out && misaligned(depth32_out[s], 3u)) DI_REFUSE("depth32_out must be 4-byte aligned");
    }
#undef DI_REFUSE
    DiCall call{};
    call.record = record_out_dev;
    call.x0 = x0, call.y0 = y0, call.step_x = step_x, call.step_y = step_y, call.grid_w = grid_w, call.grid_h = grid_h;
    call.tiles_x = (grid_w + kTileW - 1) / kTileW;
    call.tiles_y = (grid_h + kTileH - 1) / kTileH;
    call.force_coop = di->force_coop;
    const int64_t tiles = (int64_t)call.tiles_x * call.tiles_y;  // (<= max_tiles: the grid lies inside the image)
    if (tiles > di->max_tiles) return refuse(MLD_ERR_INVALID_ARG, "grid_w, grid_h: the grid has more tiles than the image");
    for (int s = 0; s < S; s++) {
        DiSeq& q = di->ring.stage[(size_t)s];
        q = DiSeq{};
        q.map = map[s];
        q.index = index[s];
        q.cam = cam[s];
        q.has_plane = (c.useRoad && coeffs && mask_dev && mask_dev[s]) ? 1 : 0;
        q.mask = q.has_plane ? mask_dev[s] : nullptr;
        q.depth = depth_out ? depth_out[s] : nullptr;
        q.depth32 = depth32_out ? depth32_out[s] : nullptr;
        q.type = type_out ? type_out[s] : nullptr;
        if (q.has_plane) {
            for (int t = 0; t < 4; t++) q.coeffs[t] = coeffs[4 * (size_t)s + t];
            // :289-291 prior = Hyperplane(normalize(a, b, c), d), as mld_set_ground_plane forms it
            double a = (double)q.coeffs[0], b = (double)q.coeffs[1], cc = (double)q.coeffs[2];
            const double z = a * a + (b * b + cc * cc);
            if (z > 0.0) {
                const double nrm = std::sqrt(z);
                a /= nrm;
                b /= nrm;
                cc /= nrm;
            }
            q.prior_n[0] = a, q.prior_n[1] = b, q.prior_n[2] = cc;
            q.prior_off = (double)q.coeffs[3];
        }
        q.index_len = (int32_t)index_len[s];
        q.n_points = (int32_t)n_points[s];
    }
    MLD_HIP(di, hipSetDevice(di->device));
    const int rc = di->ring.upload(di);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((int64_t)S * tiles);
    hipLaunchKernelGGL(k_depth_image_lane, dim3(blocks), dim3(kBlock), 0, di->stream, di->ring.d_desc.get(), c, call, di->d_over.get(), di->d_part.get());
    MLD_HIP(di, hipGetLastError());
    hipLaunchKernelGGL(k_depth_image_coop, dim3(blocks * kWaves), dim3(kWave), di->lds_bytes, di->stream, di->ring.d_desc.get(), c, call,
                       di->d_over.get(), di->d_part.get());
    MLD_HIP(di, hipGetLastError());
    hipLaunchKernelGGL(k_depth_image_finish, dim3((unsigned)S), dim3(kBlock), 0, di->stream, di->ring.d_desc.get(), call, di->d_part.get());
    MLD_HIP(di, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
