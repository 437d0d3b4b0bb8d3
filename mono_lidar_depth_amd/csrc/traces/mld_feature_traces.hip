// mld_feature_traces.hip — why a feature got the depth it got, for a batch of sequences in one call (include/mld.h,
// "mld_feature_traces"): the record the reference calls DepthCalcStatsSinglePoint (do_debug_singleFeatures,
// DepthCalcStatsSinglePoint.h:20-67: neighbours, segmented points, histogram borders, plane) and the triangle corners of
// getCloudTriangleCorners / ActivateDebugMode (DepthEstimator.cpp:348-350, PlaneEstimationCalcMaxSpanningTriangle.cpp:
// 20-35).  The inputs are the arrays mld_projected_clouds_export_device writes (pixel map, _pointIndex, camera-frame
// cloud) and, optionally, the plane mld_semantic_planes / mld_ransac_planes leave on the device.  No frame slot is
// involved, nothing is allocated per call and nothing comes back to the host.
//
// Two launches: the descriptor upload and
//   k_feature_trace   grid (sequence, feature), ONE WAVEFRONT PER FEATURE, any window up to kMaxCells cells:
//     B2  the lanes scan the window's cells in row-major order; ballot + prefix popcount give the ordered neighbour list
//         in LDS (visible index, camera-frame point)                                   NeighborFinderPixel.cpp:60-95
//     B3  the histogram's bins from ballots over the list, the scan for the first local maximum on the scalar side, the
//         kept points compacted in place                                               HistogramPointDepth.cpp:15-123
//     B5  the farthest pair: row i of the pair matrix spread over the lanes, every lane keeps (largest distance,
//         smallest i * n + j), one (value descending, id ascending) reduction; the third corner likewise
//                                                           PlaneEstimationCalcMaxSpanningTriangle.cpp:37-100
//     B6  the serial tail - planarity, viewing ray, Hyperplane::Through, intersection, thresholds - on wave-uniform
//         values; the record is staged in LDS by lane 0 and leaves as one store of a dword per lane
//     road  the wide window as B2, then per neighbour the f32 point-to-plane distance after the f64 Tinv transform and the
//         mask bit of its original index                                               DepthEstimator.cpp:782-900
// The road fit itself is not repeated: its depth is the depth path's business.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, V3 and the size limits:
// ../batch/mld_batch_device.h).  The records are nevertheless bit for bit what
// that path and the CPU restatement compute (tests/test_feature_traces_gpu.py pins that): the device functions below
// are copies, operation for operation, of that path's arithmetic (plane_through, viewing_ray, intersect, the histogram,
// the triangle search, the thresholds), Tinv and Kinv are formed as mld_create forms them, and this unit is compiled
// without contraction like the rest of the library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"
#include "../../../include/mld.h"

namespace {

using namespace mld_batch;

constexpr int kMaxCells = 1024;        // cells of the widest window an object accepts = entries of a list in LDS
constexpr int kMaxGridY = 65535;       // features of a sequence beyond it share blocks (grid-stride)
constexpr int kNone = 0x7fffffff;      // "no candidate yet" of the (value, id) reductions
constexpr double kDblMax = 1.7976931348623157e308;

static_assert(sizeof(mld_feature_trace) == 184, "184 bytes per record (include/mld.h)");
static_assert(offsetof(mld_feature_trace, main_depth) == 56 && offsetof(mld_feature_trace, corners) == 112,
              "field offsets of the record (include/mld.h)");
constexpr int kRecWords = (int)(sizeof(mld_feature_trace) / 4);  // 46: one dword per lane

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct TrSeq {
    const void* u;         // uv, 2 x n_feat f64 (collect_device); u, n_feat f32 (collect_tracks_device)
    const float* v;        // tracks form only
    const int32_t* map;    // W * H: visible index or -1
    const int32_t* index;  // index_len: original index of a visible point
    const double* cam;     // 3 x n_points
    const uint32_t* mask;  // ceil(n_points / 32) words, or null: the sequence has no plane
    mld_feature_trace* trace;
    int32_t* nb;           // the four lists: list_capacity x n_feat each, or null
    int32_t* seg;
    int32_t* road;
    int32_t* road_inl;
    float coeffs[4];
    int32_t n_feat;
    int32_t index_len;
    int32_t n_points;
    int32_t pad_;
};
static_assert(sizeof(TrSeq) == 120, "120 bytes per sequence (include/mld.h, DESIGN.md)");

struct TrCalib {
    double Tinv[12];  // camera -> lidar (DepthEstimator.cpp:44)
    double Kinv[9];   // intrinsics.inverse() (camera_pinhole.h:65)
    double halfX1, halfY1, halfX2, halfY2;
    double binW, thrG_min, thrG_max, thrL_val, planarThr, orthThr, roadDistThr;
    int32_t W, H, cap;
    uint32_t countMin;
    int32_t minCount, useHist, thrG_en, thrG_mode, thrL_en, thrL_mode, thrL_type, useTriMax, checkPlanar, cutBehind, useRoad;
};

__device__ __forceinline__ int prefix_count(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

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

// Eigen fixed-size Vector3d semantics: redux over three is func(x0, func(x1, x2))
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 vscale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 vdivs(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ double vdot(V3 a, V3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
__device__ __forceinline__ double vsqnorm(V3 a) { return a.x * a.x + (a.y * a.y + a.z * a.z); }
__device__ __forceinline__ double vnorm(V3 a) { return sqrt(vsqnorm(a)); }
__device__ __forceinline__ V3 vnormalized(V3 a) {
    const double z = vsqnorm(a);
    if (z > 0.0) return vdivs(a, sqrt(z));
    return a;
}
__device__ __forceinline__ V3 vcross(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// Cyclic Jacobi eigen-decomposition of a symmetric 3x3 (s = xx, xy, xz, yy, yz, zz): the eigenvector of the smallest
// eigenvalue.  Only the degenerate branch of plane_through comes here.  (Inlined: as a call it costs the kernel a stack.)
__device__ __forceinline__ V3 smallest_eigvec3(const double s[6]) {
    double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 64; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (!(off > 1e-300) || off <= 1e-32 * diag) break;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = cs * akp - sn * akq;
                    a[k][q] = sn * akp + cs * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = cs * apk - sn * aqk;
                    a[q][k] = sn * apk + cs * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
    // the first of the smallest diagonal entries, as a stable ascending sort picks it
    const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
    int i0 = 0;
    double dm = d0;
    if (d1 < dm) {
        dm = d1;
        i0 = 1;
    }
    if (d2 < dm) i0 = 2;
    V3 n0;
    n0.x = (i0 == 0) ? v[0][0] : ((i0 == 1) ? v[0][1] : v[0][2]);
    n0.y = (i0 == 0) ? v[1][0] : ((i0 == 1) ? v[1][1] : v[1][2]);
    n0.z = (i0 == 0) ? v[2][0] : ((i0 == 1) ? v[2][1] : v[2][2]);
    return n0;
}

struct Plane {
    V3 n;
    double offset;
};

// Eigen::Hyperplane<double,3>::Through (call site LinePlaneIntersectionBase.cpp:41)
__device__ __forceinline__ Plane plane_through(V3 p0, V3 p1, V3 p2) {
    const V3 v0 = vsub(p2, p0), v1 = vsub(p1, p0);
    const V3 n = vcross(v0, v1);
    const double nn = vnorm(n);
    Plane r;
    if (nn <= vnorm(v0) * vnorm(v1) * 2.220446049250313e-16) {
        // degenerate triangle: smallest eigenvector of m^T m, m = [v0^T; v1^T]
        const double s[6] = {v0.x * v0.x + v1.x * v1.x, v0.x * v0.y + v1.x * v1.y, v0.x * v0.z + v1.x * v1.z,
                             v0.y * v0.y + v1.y * v1.y, v0.y * v0.z + v1.y * v1.z, v0.z * v0.z + v1.z * v1.z};
        r.n = smallest_eigvec3(s);
    } else {
        r.n = vdivs(n, nn);
    }
    r.offset = -vdot(p0, r.n);
    return r;
}

// CameraPinhole::getViewingRays (camera_pinhole.h:52-69) + the flip (DepthEstimator.cpp:938-939)
__device__ __forceinline__ V3 viewing_ray(const TrCalib& c, double u, double v) {
    V3 d = {(c.Kinv[0] * u + c.Kinv[1] * v) + c.Kinv[2], (c.Kinv[3] * u + c.Kinv[4] * v) + c.Kinv[5],
            (c.Kinv[6] * u + c.Kinv[7] * v) + c.Kinv[8]};
    d = vnormalized(d);
    if (d.z < 0) d = vscale(d, -1.0);
    return d;
}

// LinePlaneIntersection{OrthogonalTreshold,Normal}::GetIntersection
__device__ __forceinline__ bool intersect(const TrCalib& c, bool orth, Plane pl, V3 n0, V3 n1, double& depth) {
    if (orth) {
        const V3 ln = vnormalized(n1), pn = vnormalized(pl.n);
        if (!(fabs(vdot(pn, ln)) >= c.orthThr)) return false;
    }
    const V3 dir = vnormalized(vsub(n1, n0));  // ParametrizedLine::Through(n0, n1)
    const double t = -(pl.offset + vdot(pl.n, n0)) / vdot(pl.n, dir);
    const V3 p = vadd(n0, vscale(dir, t));
    depth = p.z;
    return true;
}

// TresholdDepthGlobal::CheckInDepth / TresholdDepthLocal::CheckInBounds: 0 when in bounds (depth possibly adjusted) or the
// failing result type
__device__ __forceinline__ int apply_thresholds(const TrCalib& c, double minZ, double maxZ, double& depth) {
    if (c.thrG_en) {
        if (depth < c.thrG_min) {
            if (c.thrG_mode == 0) return MLD_TresholdDepthGlobalSmallerMin;
            depth = c.thrG_min;
        } else if (depth > c.thrG_max) {
            if (c.thrG_mode == 0) return MLD_TresholdDepthGlobalGreaterMax;
            depth = c.thrG_max;
        }
    }
    if (c.thrL_en) {
        const double interval = maxZ - minZ;
        double lo, hi;
        if (c.thrL_type == 1) {
            const double r = interval * c.thrL_val;
            lo = minZ - r;
            hi = maxZ + r;
        } else {
            lo = minZ - c.thrL_val;
            hi = maxZ + c.thrL_val;
        }
        if (depth < lo) {
            if (c.thrL_mode == 0) return MLD_TresholdDepthLocalSmallerMin;
            depth = lo;
        } else if (depth > hi) {
            if (c.thrL_mode == 0) return MLD_TresholdDepthLocalGreaterMax;
            depth = hi;
        }
    }
    return 0;
}

// The lists of the feature a wavefront works on, c.cap entries each (dynamic LDS).
struct Lists {
    double* x;     // camera-frame points of the current list (the neighbours, then the segmented points in place)
    double* y;
    double* z;
    int32_t* vis;  // visible index of neighbour i
    int32_t* aux;  // the histogram's bin of neighbour i; in the road stage its original index
    int32_t* pos;  // positions of the segmented points in the neighbour list; in the road stage those of the inliers
};

// Window scan (NeighborFinderPixel.cpp:60-95) + 3-D gather (NeighborFinderBase.cpp:15-27): the neighbours in the
// reference's row-major scan order; their count (wave-uniform, <= c.cap because the window has at most that many cells).
// Bounds in f64 with (int) truncation, as there.  A cell whose map value or index lies outside the arrays counts as empty
// and sets `bad`.  row: where the visible indices go (up to list_cap of them), or null.
__device__ __forceinline__ int gather_window(const TrCalib& c, const TrSeq& q, double u, double v, double halfX, double halfY,
                                             const Lists& L, int lane, MLD_BATCH_GLOBAL int32_t* row, int list_cap, bool& bad) {
    if (!(isfinite(u) && isfinite(v))) return 0;  // reference: undefined behaviour (int cast of NaN)
    double a;
    a = u - halfX;
    const double left = (a < 0.) ? 0. : a;  // std::max(a, 0.)
    a = u + halfX;
    const double right = ((double)(c.W - 1) < a) ? (double)(c.W - 1) : a;  // std::min(a, W - 1)
    a = v - halfY;
    const double top = (a < 0.) ? 0. : a;
    a = v + halfY;
    const double bottom = ((double)(c.H - 1) < a) ? (double)(c.H - 1) : a;
    const int x0 = uniform((int)left), x1 = uniform((int)right), y0 = uniform((int)top), y1 = uniform((int)bottom);
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    if (nx <= 0 || ny <= 0) return 0;
    if (x0 < 0 || y0 < 0 || x1 >= c.W || y1 >= c.H) return 0;  // unreachable for finite features
    if ((long long)nx * (long long)ny > (long long)c.cap) return 0;  // unreachable: the object's bound on the window
    const int ncell = nx * ny;
    const MLD_BATCH_GLOBAL int32_t* map = as_global(q.map);
    const MLD_BATCH_GLOBAL int32_t* index = as_global(q.index);
    const MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    int k = 0;
    bool badl = false;
    for (int base = 0; base < ncell; base += kWave) {
        const int cidx = base + lane;
        int m = -1;
        if (cidx < ncell) {
            const int r = cidx / nx, col = cidx - r * nx;
            m = map[(size_t)(x0 + col) + (size_t)(y0 + r) * (size_t)c.W];
        }
        bool has = false;
        int orig = 0;
        if (m != -1) {
            if (m < 0 || m >= q.index_len) {
                badl = true;
            } else {
                orig = index[m];
                if (orig < 0 || orig >= q.n_points)
                    badl = true;
                else
                    has = true;
            }
        }
        const unsigned long long mk = __ballot(has);
        const int rank = k + prefix_count(mk);
        if (has && rank < c.cap) {
            L.x[rank] = cam[3 * (size_t)orig];
            L.y[rank] = cam[3 * (size_t)orig + 1];
            L.z[rank] = cam[3 * (size_t)orig + 2];
            L.vis[rank] = m;
            L.aux[rank] = orig;
            if (row && rank < list_cap) row[rank] = m;
        }
        k += (int)__popcll(mk);
    }
    if (__ballot(badl) != 0ull) bad = true;
    k = uniform(k);
    return k < c.cap ? k : c.cap;
}

// PointHistogram::FilterPointsMinDistBlob (HistogramPointDepth.cpp:15-123, Histogram.cpp:14-49) on the first k list entries:
// the points of the first local-maximum bin, compacted in place, their positions in L.pos.  Returns their count or -1;
// lower / higher: the borders of the chosen bin (-1 without one).
__device__ __forceinline__ int hist_segment(const TrCalib& c, int k, const Lists& L, int lane, double& lower, double& higher) {
    lower = -1.0;
    higher = -1.0;
    int md = 0;  // :36-41: the largest ceil(depth) above 0
    for (int i = lane; i < k; i += kWave) {
        double d = L.z[i];
        d = (999. < d) ? 999. : d;  // DepthEstimator.cpp:743
        if (d > (double)md) md = (int)ceil(d);
    }
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) md = max(md, __shfl_xor(md, s));
    md = uniform(md);
    const int binCount = (int)((double)md / c.binW + 1.0);  // :43
    if (binCount <= 1) return -1;                           // :53
    int bmin = kNone;
    for (int i = lane; i < k; i += kWave) {
        double d = L.z[i];
        d = (999. < d) ? 999. : d;
        const double value = (1e10 < d) ? 1e10 : d;  // Histogram.cpp:29
        const double qd = fabs(value / c.binW);
        const double lim = (double)binCount - 1.;
        const int bi = (int)((lim < qd) ? lim : qd);  // Histogram.cpp:30
        L.aux[i] = bi;
        bmin = min(bmin, bi);
    }
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) bmin = min(bmin, __shfl_xor(bmin, s));
    bmin = uniform(bmin);
    __syncthreads();
    // HistogramPointDepth.cpp:70-85, started at the first non-empty bin (the empty bins ahead of it change nothing)
    int binMaxId = -1, binMaxVal = -1, binValue = 0;
    for (int i = bmin; i < binCount; i++) {
        const int last = binValue;
        int cnt = 0;
        for (int b = 0; b < k; b += kWave) {
            const int e = b + lane;
            cnt += (int)__popcll(__ballot(e < k && L.aux[e] == i));
        }
        binValue = uniform(cnt);
        if ((binValue > binMaxVal) && (binValue >= c.minCount)) {
            binMaxVal = binValue;
            binMaxId = i;
        } else if (binValue < binMaxVal)
            break;
        if ((last > 0) && (binValue == 0)) return -1;
    }
    if (binMaxId < 0) return -1;                           // :95
    lower = (double)binMaxId * c.binW - 0.0 * c.binW;      // :99
    higher = (double)binMaxId * c.binW + 1.0 * c.binW;     // :100
    int kk = 0;
    for (int b = 0; b < k; b += kWave) {  // :115-120
        const int i = b + lane;
        bool keep = false;
        double x = 0, y = 0, z = 0;
        if (i < k) {
            z = L.z[i];
            const double d = (999. < z) ? 999. : z;
            keep = (d >= lower) && (d < higher);
            x = L.x[i];
            y = L.y[i];
        }
        const unsigned long long m = __ballot(keep);
        const int rank = kk + prefix_count(m);  // (<= i: a lane writes at or below what this pass has read)
        if (keep) {
            L.x[rank] = x;
            L.y[rank] = y;
            L.z[rank] = z;
            L.pos[rank] = i;
        }
        kk += (int)__popcll(m);
    }
    return uniform(kk);
}

__device__ __forceinline__ V3 list_point(const Lists& L, int i) { return {L.x[i], L.y[i], L.z[i]}; }

// PlaneEstimationCalcMaxSpanningTriangle::CalculatePlaneCorners (PlaneEstimationCalcMaxSpanningTriangle.cpp:37-100) with
// _distTreshold = 0 on the first n list entries.  The serial loops' strict '>' keeps the FIRST maximal pair in (i, j)
// order and the first maximal k: the smallest id among the candidates at the maximum.
__device__ __forceinline__ bool max_spanning_triangle(int n, const Lists& L, int lane, int& ci, int& cj, int& ck) {
    if (n < 3) return false;
    double bd = -1.0;
    int bid = kNone;
    for (int i = 0; i < n - 1; i++) {
        const V3 pi = list_point(L, i);
        for (int j = i + 1 + lane; j < n; j += kWave) {
            const double d = vsqnorm(vsub(pi, list_point(L, j)));
            const int id = i * n + j;
            if (d > bd || (d == bd && id < bid)) {
                bd = d;
                bid = id;
            }
        }
    }
    reduce_best(bd, bid);
    bid = uniform(bid);
    if (bid == kNone || bd <= 0.0) return false;  // :65
    const int bi = bid / n, bj = bid - (bid / n) * n;
    const V3 pa = list_point(L, bi), pb = list_point(L, bj);
    double b2 = -1.0;
    int bk = kNone;
    for (int kx = lane; kx < n - 1; kx += kWave) {  // :71 the last point is never considered
        if (kx == bi || kx == bj) continue;
        const V3 pk = list_point(L, kx);
        const double d1 = vsqnorm(vsub(pk, pa));
        if (d1 <= 0.0) continue;
        const double d2 = vsqnorm(vsub(pk, pb));
        if (d2 <= 0.0) continue;
        const double d = d1 + d2;
        if (d > b2) {  // (kx ascends: the first of a lane's equals stays)
            b2 = d;
            bk = kx;
        }
    }
    reduce_best(b2, bk);
    bk = uniform(bk);
    if (bk == kNone) return false;
    ci = bi;
    cj = bj;
    ck = bk;
    return true;
}

// min / max of z over the first n list entries as the serial loop leaves them (TresholdDepthLocal.cpp:23-29): strict
// comparisons from +-DBL_MAX, so a NaN never enters and the first of equal values stays.
__device__ __forceinline__ void list_minmax_z(int n, const Lists& L, int lane, double& mn, double& mx) {
    double a = -kDblMax, b = -kDblMax;  // the largest -z and the largest z so far
    int ia = kNone, ib = kNone;
    for (int i = lane; i < n; i += kWave) {
        const double z = L.z[i];
        if (-z > a) {
            a = -z;
            ia = i;
        }
        if (z > b) {
            b = z;
            ib = i;
        }
    }
    reduce_best(a, ia);
    reduce_best(b, ib);
    ia = uniform(ia);
    ib = uniform(ib);
    mn = (ia == kNone) ? kDblMax : L.z[ia];
    mx = (ib == kNone) ? -kDblMax : L.z[ib];
}

template <bool kTracks>
__device__ __forceinline__ void trace_feature(const TrCalib& c, const TrSeq& q, const Lists& L, mld_feature_trace* rec,
                                              const int f, const int lane, const int list_cap) {
    double u, v;
    if (kTracks) {  // the integer pixel the tracklet layer evaluates (std::pair<int,int>)
        u = (double)truncf(as_global(static_cast<const float*>(q.u))[f]);
        v = (double)truncf(as_global(q.v)[f]);
    } else {
        u = as_global(static_cast<const double*>(q.u))[2 * (size_t)f];
        v = as_global(static_cast<const double*>(q.u))[2 * (size_t)f + 1];
    }
    const size_t row = (size_t)f * (size_t)list_cap;
    const double nan = __builtin_nan("");
    int flags = (isfinite(u) && isfinite(v)) ? 0 : MLD_TRACE_FLAG_NONFINITE_FEATURE;
    bool bad = false;

    // ---- B2: the narrow window (DepthEstimator.cpp:509, scale 1.0 x 1.0) ----
    const int n_nb = gather_window(c, q, u, v, c.halfX1, c.halfY1, L, lane, q.nb ? as_global(q.nb) + row : nullptr, list_cap, bad);
    __syncthreads();
    int main_type = MLD_Unspecified, n_seg = 0;
    int cp0 = -1, cp1 = -1, cp2 = -1, cv0 = -1, cv1 = -1, cv2 = -1;
    double main_depth = -1.0, lower = -1.0, higher = -1.0;
    Plane pl = {{nan, nan, nan}, nan};
    V3 c1 = {nan, nan, nan}, c2 = c1, c3 = c1;
    if ((unsigned)n_nb < c.countMin) {  // :680, compared as unsigned
        main_type = MLD_RadiusSearchInsufficientPoints;
    } else {
        // ---- B3: CalculateDepthSegmentation (:726-780) ----
        int ks = n_nb;
        if (c.useHist) {
            ks = hist_segment(c, n_nb, L, lane, lower, higher);
        } else {
            for (int i = lane; i < n_nb; i += kWave) L.pos[i] = i;
        }
        __syncthreads();
        if (ks < 0) {
            main_type = MLD_HistogramNoLocalMax;
        } else {
            n_seg = ks;
            if (q.seg) {
                MLD_BATCH_GLOBAL int32_t* out = as_global(q.seg) + row;
                const int m = ks < list_cap ? ks : list_cap;
                for (int i = lane; i < m; i += kWave) out[i] = L.pos[i];
            }
            // ---- B5: the corners (:915-926) ----
            bool ok = true;
            int ci = 0, cj = 1, ck = 2;
            if (c.useTriMax) {
                ok = max_spanning_triangle(ks, L, lane, ci, cj, ck);
                if (!ok) main_type = MLD_TriangleNotPlanarInsufficientPoints;
            } else if (ks < 3) {
                ok = false;
                main_type = MLD_HistogramNoLocalMax;  // :920-921
            }
            if (ok) {
                // ---- B6: the tail of CalculateDepthSegmented (:928-1036), on wave-uniform values ----
                cp0 = ci, cp1 = cj, cp2 = ck;
                cv0 = L.vis[L.pos[ci]], cv1 = L.vis[L.pos[cj]], cv2 = L.vis[L.pos[ck]];
                c1 = list_point(L, ci), c2 = list_point(L, cj), c3 = list_point(L, ck);
                double mn, mx;
                list_minmax_z(ks, L, lane, mn, mx);
                int type = MLD_Success;
                double depth = -1.0;
                if (c.checkPlanar) {  // PlaneEstimationCheckPlanar.cpp:18-44
                    const V3 e1 = vnormalized(vsub(c2, c1)), e2 = vnormalized(vsub(c3, c1)), e3 = vnormalized(vsub(c3, c2));
                    const double l12 = vnorm(vcross(e1, e2)), l13 = vnorm(vcross(e1, e3)), l23 = vnorm(vcross(e2, e3));
                    if (!((l12 >= c.planarThr) && (l13 >= c.planarThr) && (l23 >= c.planarThr))) type = MLD_TriangleNotPlanar;
                }
                if (type == MLD_Success) {
                    const V3 dir = viewing_ray(c, u, v);
                    const V3 support = {0, 0, 0};
                    pl = plane_through(c1, c2, c3);
                    if (!intersect(c, c.orthThr > 0 /* DepthEstimator.cpp:77-81 */, pl, support, dir, depth))
                        type = MLD_PlaneViewrayNotOrthogonal;
                }
                if (type == MLD_Success) {
                    const int t = apply_thresholds(c, mn, mx, depth);
                    if (t) type = t;
                }
                if (type == MLD_Success && depth < 0 && c.cutBehind) type = MLD_CornerBehindCamera;
                main_type = type;
                main_depth = (type == MLD_Success) ? depth : -1.0;
            }
        }
    }
    __syncthreads();  // (the lists are rewritten from here)

    // ---- the road fallback (:578-597): the wide window, the distance test, the mask ----
    int road_state = MLD_TRACE_ROAD_NOT_REACHED, n_road = 0, n_inl = 0;
    if (c.useRoad && q.mask && main_type != MLD_Success && main_type != MLD_RadiusSearchInsufficientPoints) {
        n_road = gather_window(c, q, u, v, c.halfX2, c.halfY2, L, lane, q.road ? as_global(q.road) + row : nullptr, list_cap, bad);
        __syncthreads();
        if ((unsigned)n_road < c.countMin) {  // :585-586
            road_state = MLD_TRACE_ROAD_FEW_NEIGHBOURS;
        } else {
            // CalculateDepthSegmentationPlane (:782-900)
            const MLD_BATCH_GLOBAL uint32_t* mask = as_global(q.mask);
            bool anyFar = false;
            int kk = 0;
            for (int b = 0; b < n_road; b += kWave) {
                const int i = b + lane;
                bool far = false, inl = false;
                if (i < n_road) {
                    const double x = L.x[i], y = L.y[i], z = L.z[i];
                    const int orig = L.aux[i];
                    // :810 T_lidar_cam * p (fixed-size product order), :811 float, :812 float plane distance
                    const double xl = c.Tinv[3] + (c.Tinv[0] * x + (c.Tinv[1] * y + c.Tinv[2] * z));
                    const double yl = c.Tinv[7] + (c.Tinv[4] * x + (c.Tinv[5] * y + c.Tinv[6] * z));
                    const double zl = c.Tinv[11] + (c.Tinv[8] * x + (c.Tinv[9] * y + c.Tinv[10] * z));
                    const float xf = (float)xl, yf = (float)yl, zf = (float)zl;
                    const float d = fabsf(q.coeffs[0] * xf + q.coeffs[1] * yf + q.coeffs[2] * zf + q.coeffs[3]);
                    far = (double)d > c.roadDistThr;                          // :814-815
                    inl = (mask[(unsigned)orig >> 5] >> ((unsigned)orig & 31u)) & 1u;  // :817 CheckPointInPlane
                }
                anyFar = anyFar || (__ballot(far) != 0ull);
                const unsigned long long m = __ballot(inl);
                const int rank = kk + prefix_count(m);
                if (inl) L.pos[rank] = i;
                kk += (int)__popcll(m);
            }
            kk = uniform(kk);
            __syncthreads();
            if (anyFar) {
                road_state = MLD_TRACE_ROAD_FAR_NEIGHBOUR;  // (the reference leaves at the first far neighbour: no list)
            } else {
                n_inl = kk;
                road_state = kk < 3 ? MLD_TRACE_ROAD_FEW_INLIERS : MLD_TRACE_ROAD_FIT;  // :827-829
                if (q.road_inl) {
                    MLD_BATCH_GLOBAL int32_t* out = as_global(q.road_inl) + row;
                    const int m = kk < list_cap ? kk : list_cap;
                    for (int i = lane; i < m; i += kWave) out[i] = L.pos[i];
                }
            }
        }
    }
    if (bad) flags |= MLD_TRACE_FLAG_BAD_INPUT;

    // ---- the record: staged by lane 0, stored as one dword per lane ----
    if (lane == 0) {
        rec->main_type = main_type;
        rec->road_state = road_state;
        rec->n_nb = n_nb;
        rec->n_seg = n_seg;
        rec->n_road = n_road;
        rec->n_road_inl = n_inl;
        rec->corner_pos[0] = cp0, rec->corner_pos[1] = cp1, rec->corner_pos[2] = cp2;
        rec->corner_vis[0] = cv0, rec->corner_vis[1] = cv1, rec->corner_vis[2] = cv2;
        rec->flags = flags;
        rec->pad_ = 0;
        rec->main_depth = main_depth;
        rec->hist_lower = lower;
        rec->hist_higher = higher;
        rec->plane_n[0] = pl.n.x, rec->plane_n[1] = pl.n.y, rec->plane_n[2] = pl.n.z;
        rec->plane_offset = pl.offset;
        rec->corners[0] = c1.x, rec->corners[1] = c1.y, rec->corners[2] = c1.z;
        rec->corners[3] = c2.x, rec->corners[4] = c2.y, rec->corners[5] = c2.z;
        rec->corners[6] = c3.x, rec->corners[7] = c3.y, rec->corners[8] = c3.z;
    }
    __syncthreads();
    if (lane < kRecWords)
        as_global(reinterpret_cast<uint32_t*>(q.trace + f))[lane] = reinterpret_cast<const uint32_t*>(rec)[lane];
    __syncthreads();  // (the next feature of this block rewrites the lists and the staged record)
}

// Grid (sequence, feature); one wavefront per block.  Dynamic LDS: the lists (36 bytes per entry of c.cap, an even number)
// and the staged record behind them.
template <bool kTracks>
__global__ __launch_bounds__(kWave) void k_feature_trace(const TrSeq* __restrict__ desc, TrCalib c, int list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const TrSeq q = desc[blockIdx.x];
    const int lane = (int)threadIdx.x;
    Lists L;
    L.x = reinterpret_cast<double*>(smem);
    L.y = L.x + c.cap;
    L.z = L.y + c.cap;
    L.vis = reinterpret_cast<int32_t*>(L.z + c.cap);
    L.aux = L.vis + c.cap;
    L.pos = L.aux + c.cap;
    mld_feature_trace* rec = reinterpret_cast<mld_feature_trace*>(L.pos + c.cap);
    for (int f = (int)blockIdx.y; f < q.n_feat; f += (int)gridDim.y)  // (uniform in the block)
        trace_feature<kTracks>(c, q, L, rec, f, lane, list_cap);
}

char g_error[512] = "";  // refusals without an object: mld_feature_traces_last_error(NULL)

// 3x3 inverse by cofactors (Eigen compute_inverse<Matrix3d>): result(i,j) = cofactor<j,i> / det.
double cof(const double m[9], int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
void inverse3(const double m[9], double out[9]) {
    const double c0 = cof(m, 0, 0), c1 = cof(m, 1, 0), c2 = cof(m, 2, 0);
    const double det = c0 * m[0] + (c1 * m[3] + c2 * m[6]);
    const double invdet = 1.0 / det;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[i * 3 + j] = cof(m, j, i) * invdet;
}

// Upper bound on the cells a window can cover: floor(2 half) + 2 columns / rows, and no more than the image has.
double window_cells(double halfX, double halfY, int W, int H) {
    double nx = std::floor(2.0 * halfX) + 2.0, ny = std::floor(2.0 * halfY) + 2.0;
    if (nx > (double)W) nx = (double)W;
    if (ny > (double)H) ny = (double)H;
    return nx * ny;
}

// What mld_create refuses of a parameter set, a camera and a transform, with its texts; and what only this object refuses.
int refuse_config(const mld_params& P, const mld_camera& cam, const double T[12], std::string& why) {
    if (P.do_use_PCA) {
        why = "do_use_PCA: the eigen-solve is a tolerance path, the trace promises equality";
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    if (P.neighbor_search_mode != 0) {
        why = "neighbor_search_mode has the invalid value: " + std::to_string(P.neighbor_search_mode);  // :57
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    if (P.do_use_depth_segmentation) {
        why = "DepthEstimator: Region growing not supported!";  // :608
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    if (P.do_use_ransac_plane) {
        if (P.plane_estimator_use_triangle_maximation) {
        } else if (P.plane_estimator_use_leastsquares) {
            why = "plane_estimator_use_leastsquares (Ceres variant) is not supported";
            return MLD_ERR_UNSUPPORTED_MODE;
        } else if (P.plane_estimator_use_mestimator) {
        } else {
            why = "No road depth estimator selected.";  // :94
            return MLD_ERR_NO_ROAD_ESTIMATOR;
        }
    }
    if (P.pixelarea_search_witdh < 0 || P.pixelarea_search_height < 0) {
        why = "negative search window";
        return MLD_ERR_INVALID_ARG;
    }
    if (cam.width < 1 || cam.height < 1) {
        why = "bad image size";
        return MLD_ERR_INVALID_ARG;
    }
    if (cam.width > 65535 || cam.height > 65535 || (int64_t)cam.width * cam.height > (int64_t)1 << 30) {
        why = "image larger than 65535 pixels on a side or 2^30 pixels in all";
        return MLD_ERR_CAPACITY;
    }
    if (!std::isfinite(cam.focal_length) || cam.focal_length == 0.0 || !std::isfinite(cam.principal_point_x) ||
        !std::isfinite(cam.principal_point_y)) {
        why = "bad camera intrinsics";
        return MLD_ERR_INVALID_ARG;
    }
    for (int t = 0; t < 12; t++)
        if (!std::isfinite(T[t])) {
            why = "non-finite lidar->camera transform";
            return MLD_ERR_INVALID_ARG;
        }
    const double halfX2 = (double)P.pixelarea_search_witdh * 0.5 * (double)2.0f;
    const double halfY2 = (double)P.pixelarea_search_height * 0.5 * (double)1.5f;
    if (window_cells(halfX2, halfY2, cam.width, cam.height) > (double)kMaxCells) {
        why = "the wide window (2.0 x 1.5 the search area) can cover more than 1024 cells";
        return MLD_ERR_CAPACITY;
    }
    return MLD_OK;
}

void build_calib(TrCalib& c, const mld_params& P, const mld_camera& cam, const double T[12]) {
    // _transform_cam_to_lidar = transform_lidar_to_cam.inverse()   (DepthEstimator.cpp:44), as mld_create forms it
    const double Lm[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    double Li[9];
    inverse3(Lm, Li);
    const double t[3] = {T[3], T[7], T[11]};
    for (int i = 0; i < 3; i++) {
        c.Tinv[i * 4 + 0] = Li[i * 3 + 0];
        c.Tinv[i * 4 + 1] = Li[i * 3 + 1];
        c.Tinv[i * 4 + 2] = Li[i * 3 + 2];
        c.Tinv[i * 4 + 3] = (-Li[i * 3 + 0]) * t[0] + ((-Li[i * 3 + 1]) * t[1] + (-Li[i * 3 + 2]) * t[2]);
    }
    const double K[9] = {cam.focal_length, 0, cam.principal_point_x, 0, cam.focal_length, cam.principal_point_y, 0, 0, 1};
    inverse3(K, c.Kinv);
    c.W = cam.width;
    c.H = cam.height;
    // NeighborFinderPixel.cpp:67-68, scales (1, 1) and (2.0f, 1.5f) (DepthEstimator.cpp:509,585)
    c.halfX1 = (double)P.pixelarea_search_witdh * 0.5 * (double)1.0f;
    c.halfY1 = (double)P.pixelarea_search_height * 0.5 * (double)1.0f;
    c.halfX2 = (double)P.pixelarea_search_witdh * 0.5 * (double)2.0f;
    c.halfY2 = (double)P.pixelarea_search_height * 0.5 * (double)1.5f;
    int cap = (int)window_cells(c.halfX2, c.halfY2, cam.width, cam.height);  // (contains the narrow window's)
    if (cap < 2) cap = 2;
    c.cap = (cap + 1) & ~1;
    c.binW = P.histogram_segmentation_bin_witdh;
    c.minCount = P.histogram_segmentation_min_pointcount;
    c.countMin = (unsigned)P.radiusSearch_count_min;
    c.useHist = P.do_use_histogram_segmentation;
    c.thrG_en = P.treshold_depth_enabled;
    c.thrG_mode = P.treshold_depth_mode;
    c.thrG_min = (double)P.treshold_depth_min;
    c.thrG_max = (double)P.treshold_depth_max;
    c.thrL_en = P.treshold_depth_local_enabled;
    c.thrL_mode = P.treshold_depth_local_mode;
    c.thrL_type = P.treshold_depth_local_valuetype;
    c.thrL_val = P.treshold_depth_local_value;
    c.useTriMax = P.do_use_triangle_size_maximation;
    c.checkPlanar = P.do_check_triangleplanar_condition;
    c.planarThr = P.triangleplanar_crossnorm_treshold;
    c.orthThr = P.viewray_plane_orthoganality_treshold;
    c.cutBehind = P.do_use_cut_behind_camera;
    c.useRoad = P.do_use_ransac_plane;
    c.roadDistThr = P.ransac_plane_point_distance_treshold;
}

}  // namespace

struct mld_feature_traces : mld_batch::Object {
    int n_seq = 0;
    int64_t max_features = 0;
    TrCalib calib{};
    size_t lds_bytes = 0;
    mld_batch::DescRing<TrSeq> ring;
};

namespace {

void free_own(mld_feature_traces*) {}

// Both collect calls: u_tab = uv (v_tab null) or u, v.
template <bool kTracks>
int collect(mld_feature_traces* ft, const char* fn, const void* const* u_tab, const float* const* v_tab, const int64_t* n_features,
            const int32_t* const* map, const int32_t* const* index, const int64_t* index_len, const double* const* cam,
            const int64_t* n_points, const float* coeffs, const uint32_t* const* mask_dev, int list_capacity,
            mld_feature_trace* const* trace_out, int32_t* const* nb_out, int32_t* const* seg_out, int32_t* const* road_out,
            int32_t* const* road_inl_out) {
    if (!ft) return no_object(g_error, fn, "ft");
    auto refuse = [&](int code, const char* text) { return fail(ft, code, (std::string(fn) + ": " + text).c_str()); };
#define TR_REFUSE(text) return refuse(MLD_ERR_INVALID_ARG, text)
    if (!u_tab) TR_REFUSE(kTracks ? "null table u" : "null table uv");
    if (kTracks && !v_tab) TR_REFUSE("null table v");
    if (!n_features) TR_REFUSE("null table n_features");
    if (!map) TR_REFUSE("null table map");
    if (!index) TR_REFUSE("null table index");
    if (!index_len) TR_REFUSE("null table index_len");
    if (!cam) TR_REFUSE("null table cam");
    if (!n_points) TR_REFUSE("null table n_points");
    if (!trace_out) TR_REFUSE("null table trace_out");
    if (list_capacity < 0 || list_capacity > kMaxCells) TR_REFUSE("list_capacity must be in 0 .. 1024");
    if ((coeffs != nullptr) != (mask_dev != nullptr)) TR_REFUSE("coeffs and mask_dev come together or not at all");
    const int S = ft->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        const int64_t n = n_features[s];
        if (n < 0) TR_REFUSE("negative n_features");
        if (index_len[s] < 0) TR_REFUSE("negative index_len");
        if (n_points[s] < 0) TR_REFUSE("negative n_points");
        if (n > ft->max_features) return refuse(MLD_ERR_CAPACITY, "n_features exceeds the max_features of the object");
        if (n_points[s] > kMaxPoints || index_len[s] > kMaxPoints)
            return refuse(MLD_ERR_CAPACITY, "n_points or index_len exceeds 8 388 607");
        if (n == 0) continue;  // (needs no arrays)
        if (!u_tab[s]) TR_REFUSE(kTracks ? "null array u of a sequence with features" : "null array uv of a sequence with features");
        if (kTracks && !v_tab[s]) TR_REFUSE("null array v of a sequence with features");
        if (!map[s]) TR_REFUSE("null array map of a sequence with features");
        if (index_len[s] > 0 && !index[s]) TR_REFUSE("null array index of a sequence with features and index_len > 0");
        if (n_points[s] > 0 && !cam[s]) TR_REFUSE("null array cam of a sequence with features and n_points > 0");
        if (!trace_out[s]) TR_REFUSE("null array trace_out of a sequence with features");
        if (kTracks) {
            if (misaligned(u_tab[s], 3u)) TR_REFUSE("u must be 4-byte aligned");
            if (misaligned(v_tab[s], 3u)) TR_REFUSE("v must be 4-byte aligned");
        } else if (misaligned(u_tab[s], 7u)) {
            TR_REFUSE("uv must be 8-byte aligned");
        }
        if (misaligned(map[s], 3u)) TR_REFUSE("map must be 4-byte aligned");
        if (misaligned(index[s], 3u)) TR_REFUSE("index must be 4-byte aligned");
        if (misaligned(cam[s], 7u)) TR_REFUSE("cam must be 8-byte aligned");
        if (mask_dev && misaligned(mask_dev[s], 3u)) TR_REFUSE("mask_dev must be 4-byte aligned");
        if (misaligned(trace_out[s], 7u)) TR_REFUSE("trace_out must be 8-byte aligned");
        if (list_capacity > 0) {
            if (nb_out && misaligned(nb_out[s], 3u)) TR_REFUSE("nb_out must be 4-byte aligned");
            if (seg_out && misaligned(seg_out[s], 3u)) TR_REFUSE("seg_out must be 4-byte aligned");
            if (road_out && misaligned(road_out[s], 3u)) TR_REFUSE("road_out must be 4-byte aligned");
            if (road_inl_out && misaligned(road_inl_out[s], 3u)) TR_REFUSE("road_inl_out must be 4-byte aligned");
        }
        if (n > longest) longest = n;
    }
#undef TR_REFUSE
    for (int s = 0; s < S; s++) {
        TrSeq& q = ft->ring.stage[(size_t)s];
        q = TrSeq{};
        const int64_t n = n_features[s];
        if (n == 0) continue;
        const bool lists = list_capacity > 0;
        q.u = u_tab[s];
        q.v = kTracks ? v_tab[s] : nullptr;
        q.map = map[s];
        q.index = index[s];
        q.cam = cam[s];
        q.mask = mask_dev ? mask_dev[s] : nullptr;
        q.trace = trace_out[s];
        q.nb = (lists && nb_out) ? nb_out[s] : nullptr;
        q.seg = (lists && seg_out) ? seg_out[s] : nullptr;
        q.road = (lists && road_out) ? road_out[s] : nullptr;
        q.road_inl = (lists && road_inl_out) ? road_inl_out[s] : nullptr;
        for (int t = 0; t < 4; t++) q.coeffs[t] = (coeffs && q.mask) ? coeffs[4 * (size_t)s + t] : 0.f;
        q.n_feat = (int32_t)n;
        q.index_len = (int32_t)index_len[s];
        q.n_points = (int32_t)n_points[s];
    }
    if (longest == 0) return MLD_OK;  // nothing to trace, nothing to launch
    MLD_HIP(ft, hipSetDevice(ft->device));
    const int rc = ft->ring.upload(ft);
    if (rc) return rc;
    const unsigned gy = (unsigned)(longest < kMaxGridY ? longest : kMaxGridY);
    hipLaunchKernelGGL(k_feature_trace<kTracks>, dim3((unsigned)S, gy), dim3(kWave), ft->lds_bytes, ft->stream, ft->ring.d_desc,
                       ft->calib, list_capacity);
    MLD_HIP(ft, hipGetLastError());
    return MLD_OK;
}

}  // namespace

extern "C" {

mld_feature_traces* mld_feature_traces_create(mld_ctx* ctx, int n_seq, int64_t max_features, const mld_params* params,
                                              const mld_camera* camera, const double T_cam_lidar[12], int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_feature_traces_create: n_seq must be in 1 .. 65536";
        if (max_features < 1 || max_features > kMaxFeatures) return "mld_feature_traces_create: max_features must be in 1 .. 16777216";
        if (!ctx) return "mld_feature_traces_create: null context";
        if (!params) return "mld_feature_traces_create: null params";
        if (!camera) return "mld_feature_traces_create: null camera";
        if (!T_cam_lidar) return "mld_feature_traces_create: null T_cam_lidar";
        return nullptr;
    };
    const char* bad = refusal();
    if (!bad) {  // (what is refused with a status of its own; still nothing of the context is used)
        std::string why;
        const int code = refuse_config(*params, *camera, T_cam_lidar, why);
        if (code != MLD_OK) {
            std::snprintf(g_error, sizeof(g_error), "mld_feature_traces_create: %s", why.c_str());
            if (status_out) *status_out = code;
            return nullptr;
        }
    }
    auto init = [&](mld_feature_traces* ft) {
        ft->n_seq = n_seq;
        ft->max_features = max_features;
        build_calib(ft->calib, *params, *camera, T_cam_lidar);
        ft->lds_bytes = (size_t)ft->calib.cap * 36 + sizeof(mld_feature_trace);
        return ft->ring.allocate(ft, n_seq);
    };
    return mld_batch::create_object<mld_feature_traces>(g_error, "mld_feature_traces_create", bad, ctx, status_out, init, free_own);
}

void mld_feature_traces_destroy(mld_feature_traces* ft) { mld_batch::destroy_object(ft, free_own); }

const char* mld_feature_traces_last_error(const mld_feature_traces* ft) { return ft ? ft->err.c_str() : g_error; }

int mld_feature_traces_collect_device(mld_feature_traces* ft, const double* const* uv, const int64_t* n_features,
                                      const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                      const double* const* cam, const int64_t* n_points, const float* coeffs,
                                      const uint32_t* const* mask_dev, int list_capacity, mld_feature_trace* const* trace_out,
                                      int32_t* const* nb_out, int32_t* const* seg_out, int32_t* const* road_out,
                                      int32_t* const* road_inl_out) {
    return collect<false>(ft, "mld_feature_traces_collect_device", reinterpret_cast<const void* const*>(uv), nullptr, n_features, map,
                          index, index_len, cam, n_points, coeffs, mask_dev, list_capacity, trace_out, nb_out, seg_out, road_out,
                          road_inl_out);
}

int mld_feature_traces_collect_tracks_device(mld_feature_traces* ft, const float* const* u, const float* const* v,
                                             const int64_t* n_features, const int32_t* const* map, const int32_t* const* index,
                                             const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                             const float* coeffs, const uint32_t* const* mask_dev, int list_capacity,
                                             mld_feature_trace* const* trace_out, int32_t* const* nb_out, int32_t* const* seg_out,
                                             int32_t* const* road_out, int32_t* const* road_inl_out) {
    return collect<true>(ft, "mld_feature_traces_collect_tracks_device", reinterpret_cast<const void* const*>(u), v, n_features, map,
                         index, index_len, cam, n_points, coeffs, mask_dev, list_capacity, trace_out, nb_out, seg_out, road_out,
                         road_inl_out);
}

}  // extern "C"
