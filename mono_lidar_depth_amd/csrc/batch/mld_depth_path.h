// mld_depth_path.h — the per-feature depth path of DepthEstimator::CalculateDepth (DepthEstimator.cpp:491-600) as the batch
// units on the exported clouds restate it: mld_feature_traces (one wavefront per feature), the unit of the dense images
// (its wave-cooperative route behind the window scan and the tail of its per-lane route) and the unit of the per-pixel neighbour counts (the
// window rule, the far test and the calibration).  ONE copy, so that a correction reaches every user: the results of these
// units are bit for bit what the tuned depth path (mld_kernels.hip) and the CPU restatement compute, and the functions
// below are, operation for operation, that path's arithmetic - the Eigen reduction order, the 999. clamp, the strict '>'
// tie rules.  The tuned path keeps its own copy; this header does not reach into it and includes nothing but
// mld_batch_device.h and the public header.  No kernel, no state.
//   device   the V3 algebra, smallest_eigvec3, Plane / plane_through, viewing_ray, intersect, apply_thresholds, finish_main
//            (the B6 tail); window_bounds, far_from_plane, mask_bit; over a list of points in LDS worked on by one
//            wavefront: gather_window, hist_segment, list_point, max_spanning_triangle, list_minmax_z, and main_path, which
//            strings the last four and finish_main together for a list from any neighbour search: the ONE sequence of
//            those calls among the batch units (k_feature_trace runs it behind its window scan, the unit of the
//            nearest-return depths behind its nearest-first search); and the skeleton of a unit with one wavefront per
//            feature: Lists, read_feature, store_record
//   host     DepthCalib / build_calib, inverse3, camera_to_lidar, window_halves, window_cells, window_span, what
//            mld_create refuses of a parameter set, a camera and a transform, with its texts (refuse_*), and what the
//            collect calls of the per-feature units refuse alike (FeatureTables, feature_*_fault, feature_grid)
// Every user is compiled without contraction.  The forms - values, references, a functor for what only one user stores -
// are the ones that left the kernels' code objects alone (profiles/depth_path_header.md).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mld_batch_device.h"
#include "../../../include/mld.h"

namespace mld_batch {

constexpr int kMaxCells = 1024;   // cells of the widest window an object accepts = entries of a list in LDS
constexpr int kNone = 0x7fffffff;  // "no candidate yet" of the (value, id) reductions
constexpr double kDblMax = 1.7976931348623157e308;

// What the kernels need of a parameter set, a camera and a transform (build_calib).
struct DepthCalib {
    double Tinv[12];  // camera -> lidar (DepthEstimator.cpp:44)
    double Kinv[9];   // intrinsics.inverse() (camera_pinhole.h:65)
    double halfX1, halfY1, halfX2, halfY2;
    double binW, thrG_min, thrG_max, thrL_val, planarThr, orthThr, roadDistThr;
    int32_t W, H, cap;
    uint32_t countMin;
    int32_t minCount, useHist, thrG_en, thrG_mode, thrL_en, thrL_mode, thrL_type, useTriMax, checkPlanar, cutBehind, useRoad;
};

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

// smallest_eigvec of mld_batch_device.h again: as one function k_sp_fit<0> moved 871 -> 769 instructions (profiles/feature_units.md)
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
__device__ __forceinline__ V3 viewing_ray(const DepthCalib& c, double u, double v) {
    V3 d = {(c.Kinv[0] * u + c.Kinv[1] * v) + c.Kinv[2], (c.Kinv[3] * u + c.Kinv[4] * v) + c.Kinv[5],
            (c.Kinv[6] * u + c.Kinv[7] * v) + c.Kinv[8]};
    d = vnormalized(d);
    if (d.z < 0) d = vscale(d, -1.0);
    return d;
}

// LinePlaneIntersection{OrthogonalTreshold,Normal}::GetIntersection
__device__ __forceinline__ bool intersect(const DepthCalib& c, bool orth, Plane pl, V3 n0, V3 n1, double& depth) {
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
__device__ __forceinline__ int apply_thresholds(const DepthCalib& c, double minZ, double maxZ, double& depth) {
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

// B6, the tail of CalculateDepthSegmented (DepthEstimator.cpp:928-1036), from the three corners and the min / max z of the
// segmented points on: the result type, and the depth or -1.  plane: null, or where the plane through the corners goes
// when the planarity check lets the path reach it.
__device__ __forceinline__ int finish_main(const DepthCalib& c, double u, double v, V3 c1, V3 c2, V3 c3, double mn, double mx, Plane* plane,
                                           double& out_depth) {
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
        const Plane pl = plane_through(c1, c2, c3);
        if (plane) *plane = pl;
        if (!intersect(c, c.orthThr > 0 /* DepthEstimator.cpp:77-81 */, pl, support, dir, depth)) type = MLD_PlaneViewrayNotOrthogonal;
    }
    if (type == MLD_Success) {
        const int t = apply_thresholds(c, mn, mx, depth);
        if (t) type = t;
    }
    if (type == MLD_Success && depth < 0 && c.cutBehind) type = MLD_CornerBehindCamera;
    out_depth = (type == MLD_Success) ? depth : -1.0;
    return type;
}

// NeighborFinderPixel.cpp:67-79 along one axis for the coordinate p: half size and clamping in f64, (int) truncation.  Two
// spellings of the one rule, side by side: the kernels with a pixel per lane keep their code with both bounds from one
// function, gather_window keeps k_feature_trace's with one value per call (profiles/depth_path_header.md).
__device__ __forceinline__ void window_bounds(double p, double half, int last, int& lo, int& hi) {
    double a = p - half;
    const double l = (a < 0.) ? 0. : a;  // std::max(a, 0.)
    a = p + half;
    const double r = ((double)last < a) ? (double)last : a;  // std::min(a, last)
    lo = (int)l;
    hi = (int)r;
}
__device__ __forceinline__ int window_lo(double p, double half) {
    const double a = p - half;
    return (int)((a < 0.) ? 0. : a);
}
__device__ __forceinline__ int window_hi(double p, double half, int last) {
    const double a = p + half;
    return (int)(((double)last < a) ? (double)last : a);
}

// The far test of a wide-window neighbour p (camera frame) against the plane `coeffs` (DepthEstimator.cpp:808-815).
__device__ __forceinline__ bool far_from_plane(const double (&Tinv)[12], const float (&coeffs)[4], double roadDistThr, V3 p) {
    // :810 T_lidar_cam * p (fixed-size product order), :811 float, :812 float plane distance
    const double xl = Tinv[3] + (Tinv[0] * p.x + (Tinv[1] * p.y + Tinv[2] * p.z));
    const double yl = Tinv[7] + (Tinv[4] * p.x + (Tinv[5] * p.y + Tinv[6] * p.z));
    const double zl = Tinv[11] + (Tinv[8] * p.x + (Tinv[9] * p.y + Tinv[10] * p.z));
    const float xf = (float)xl, yf = (float)yl, zf = (float)zl;
    const float d = fabsf(coeffs[0] * xf + coeffs[1] * yf + coeffs[2] * zf + coeffs[3]);
    return (double)d > roadDistThr;  // :814-815
}
// :817 CheckPointInPlane: the bit of the original index in the word that holds it, and in the plane's mask
__device__ __forceinline__ bool mask_bit(uint32_t word, int orig) { return (word >> ((unsigned)orig & 31u)) & 1u; }
__device__ __forceinline__ bool mask_bit(const uint32_t* mask, int orig) { return mask_bit(as_global(mask)[(unsigned)orig >> 5], orig); }

// ---- one wavefront on a list of camera-frame points in LDS (the neighbours, then the segmented points in place).  A
// unit's own lists extend this one.
struct PointList {
    double* x;
    double* y;
    double* z;
};

__device__ __forceinline__ V3 list_point(const PointList& L, int i) { return {L.x[i], L.y[i], L.z[i]}; }

// Window scan (NeighborFinderPixel.cpp:60-95) + 3-D gather (NeighborFinderBase.cpp:15-27) around (u, v): the neighbours in
// the reference's row-major scan order; their count (wave-uniform, <= c.cap because the window has at most that many cells).
// Bounds in f64 with (int) truncation, as there.  A cell whose map value or index lies outside the arrays counts as empty
// and sets `bad`.  q: a unit's descriptor of a sequence (map, index, cam, index_len, n_points).  keep(rank, m, orig): what a
// user stores besides the point of the neighbour at `rank`, with the visible index m and the original index orig.  (The
// cooperative route of the dense images keeps a copy of this scan, the one form that left its kernel's code alone:
// profiles/depth_path_header.md.  A correction here belongs there too.)
template <typename Seq, typename Keep>
__device__ __forceinline__ int gather_window(const DepthCalib& c, const Seq& q, double u, double v, double halfX, double halfY,
                                             const PointList& L, int lane, bool& bad, Keep keep) {
    if (!(isfinite(u) && isfinite(v))) return 0;  // reference: undefined behaviour (int cast of NaN)
    const int x0 = uniform(window_lo(u, halfX)), x1 = uniform(window_hi(u, halfX, c.W - 1));
    const int y0 = uniform(window_lo(v, halfY)), y1 = uniform(window_hi(v, halfY, c.H - 1));
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
    if (nx <= 0 || ny <= 0) return 0;
    if (x0 < 0 || y0 < 0 || x1 >= c.W || y1 >= c.H) return 0;        // unreachable for finite coordinates
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
        int o = 0;
        if (m != -1) {
            if (m < 0 || m >= q.index_len) {
                badl = true;
            } else {
                o = index[m];
                if (o < 0 || o >= q.n_points)
                    badl = true;
                else
                    has = true;
            }
        }
        const unsigned long long mk = __ballot(has);
        const int rank = k + prefix_count(mk);
        if (has && rank < c.cap) {
            L.x[rank] = cam[3 * (size_t)o];
            L.y[rank] = cam[3 * (size_t)o + 1];
            L.z[rank] = cam[3 * (size_t)o + 2];
            keep(rank, m, o);
        }
        k += (int)__popcll(mk);
    }
    if (__ballot(badl) != 0ull) bad = true;
    k = uniform(k);
    return k < c.cap ? k : c.cap;
}

// PointHistogram::FilterPointsMinDistBlob (HistogramPointDepth.cpp:15-123, Histogram.cpp:14-49) on the first k list entries:
// the points of the first local-maximum bin, compacted in place.  Returns their count or -1; lower / higher: the borders
// of the chosen bin (-1 without one).  bin: k ints of scratch (the bin of entry i); keep(rank, i): what else a user stores
// of the kept point at `rank` that was entry i.
template <typename Keep>
__device__ __forceinline__ int hist_segment(const DepthCalib& c, int k, const PointList& L, int32_t* bin, int lane, double& lower,
                                            double& higher, Keep keep) {
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
        bin[i] = bi;
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
            cnt += (int)__popcll(__ballot(e < k && bin[e] == i));
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
        bool kept = false;
        double x = 0, y = 0, z = 0;
        if (i < k) {
            z = L.z[i];
            const double d = (999. < z) ? 999. : z;
            kept = (d >= lower) && (d < higher);
            x = L.x[i];
            y = L.y[i];
        }
        const unsigned long long m = __ballot(kept);
        const int rank = kk + prefix_count(m);  // (<= i: a lane writes at or below what this pass has read)
        if (kept) {
            L.x[rank] = x;
            L.y[rank] = y;
            L.z[rank] = z;
            keep(rank, i);
        }
        kk += (int)__popcll(m);
    }
    return uniform(kk);
}

// PlaneEstimationCalcMaxSpanningTriangle::CalculatePlaneCorners (PlaneEstimationCalcMaxSpanningTriangle.cpp:37-100) with
// _distTreshold = 0 on the first n list entries.  The serial loops' strict '>' keeps the FIRST maximal pair in (i, j)
// order and the first maximal k: the smallest id among the candidates at the maximum.
__device__ __forceinline__ bool max_spanning_triangle(int n, const PointList& L, int lane, int& ci, int& cj, int& ck) {
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
__device__ __forceinline__ void list_minmax_z(int n, const PointList& L, int lane, double& mn, double& mx) {
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

// The main path of CalculateDepth behind the neighbour search (DepthEstimator.cpp:680, :726-780, :903-1036) on the first
// n_nb list entries, whichever search made the list: the count test, the histogram segmentation (the kept points
// compacted in place), the corners, B6.  What a user may want of it comes back by value; every field is wave-uniform.
struct MainPath {
    int type;          // the result type at the end of the main path
    int n_seg;         // points the segmentation kept; 0 without a segmentation that succeeded
    int ci, cj, ck;    // the corners' positions in the segmented list, -1 without corners
    double depth;      // -1 unless type == MLD_Success
    double lower, higher;  // the borders of the chosen bin, -1 without one
    Plane plane;       // Hyperplane::Through of the corners; NaN unless the path reached it
    V3 c1, c2, c3;     // the corners; NaN without corners
};
// bin: n_nb ints of scratch (hist_segment).  keep(rank, i): what a user stores of the segmented point at `rank` that was
// list entry i - called for every point of the segmented list, with the histogram off for every entry (rank == i).  A block
// is one wavefront and every lane is here (barriers); the user's stores are visible when the function returns.
template <typename Keep>
__device__ __forceinline__ MainPath main_path(const DepthCalib& c, double u, double v, int n_nb, const PointList& L, int32_t* bin,
                                              int lane, Keep keep) {
    const double nan = __builtin_nan("");
    MainPath r = {MLD_Unspecified, 0, -1, -1, -1, -1.0, -1.0, -1.0, {{nan, nan, nan}, nan}, {nan, nan, nan}, {nan, nan, nan},
                  {nan, nan, nan}};
    if ((unsigned)n_nb < c.countMin) {  // :680, compared as unsigned
        r.type = MLD_RadiusSearchInsufficientPoints;
        return r;
    }
    int ks = n_nb;  // CalculateDepthSegmentation (:726-780)
    if (c.useHist) {
        ks = hist_segment(c, n_nb, L, bin, lane, r.lower, r.higher, keep);
    } else {
        for (int i = lane; i < n_nb; i += kWave) keep(i, i);
    }
    __syncthreads();
    if (ks < 0) {
        r.type = MLD_HistogramNoLocalMax;
        return r;
    }
    r.n_seg = ks;
    int ci = 0, cj = 1, ck = 2;  // the corners (:915-926)
    if (c.useTriMax) {
        if (!max_spanning_triangle(ks, L, lane, ci, cj, ck)) {
            r.type = MLD_TriangleNotPlanarInsufficientPoints;
            return r;
        }
    } else if (ks < 3) {
        r.type = MLD_HistogramNoLocalMax;  // :920-921
        return r;
    }
    r.ci = ci, r.cj = cj, r.ck = ck;
    r.c1 = list_point(L, ci), r.c2 = list_point(L, cj), r.c3 = list_point(L, ck);
    double mn, mx;
    list_minmax_z(ks, L, lane, mn, mx);
    r.type = finish_main(c, u, v, r.c1, r.c2, r.c3, mn, mx, &r.plane, r.depth);
    return r;
}

// ---- the skeleton of a unit with one wavefront per feature and a grid of (sequence, feature)

constexpr int kMaxGridY = 65535;  // features of a sequence beyond it share blocks (grid-stride)

// The 32-bit lists of the feature a wavefront works on, beside its points (dynamic LDS; every kernel carves its own and a
// unit extends them with what only it keeps).
struct Lists : PointList {
    int32_t* vis;  // visible index of list entry i
    int32_t* aux;  // per entry, what a stage needs for a while: the original index the search leaves (of every entry, or in
                   // [0] that of the first), then the histogram's bin (main_path's `bin`)
    int32_t* pos;  // positions in the list of the points a stage keeps: the segmented points (main_path's keep(rank, i)),
                   // in a road stage the plane's inliers
};

// Feature f of a sequence from its two tables: uv in f64 (v_tab unused), or the f32 u, v of the tracklet layer truncated to
// the integer pixel it evaluates (std::pair<int,int>).
template <bool kTracks>
__device__ __forceinline__ void read_feature(const void* u_tab, const float* v_tab, int f, double& u, double& v) {
    if (kTracks) {
        u = (double)truncf(as_global(static_cast<const float*>(u_tab))[f]);
        v = (double)truncf(as_global(v_tab)[f]);
    } else {
        u = as_global(static_cast<const double*>(u_tab))[2 * (size_t)f];
        v = as_global(static_cast<const double*>(u_tab))[2 * (size_t)f + 1];
    }
}

// The exit of a record lane 0 has staged in LDS: one store of a dword per lane.  Every lane is here (barriers); behind it
// the next feature of the block may rewrite the lists and the staged record.
template <typename Rec>
__device__ __forceinline__ void store_record(const Rec* staged, Rec* out, int lane) {
    static_assert(sizeof(Rec) % 4 == 0 && sizeof(Rec) / 4 <= kWave, "one dword per lane");
    __syncthreads();
    if (lane < (int)(sizeof(Rec) / 4)) as_global(reinterpret_cast<uint32_t*>(out))[lane] = reinterpret_cast<const uint32_t*>(staged)[lane];
    __syncthreads();
}

// ---- the host side: the calibration and what is refused of it

// 3x3 inverse by cofactors (Eigen compute_inverse<Matrix3d>): result(i,j) = cofactor<j,i> / det.
inline void inverse3(const double m[9], double out[9]) {
    auto cof = [m](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
    };
    const double c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
    const double det = c0 * m[0] + (c1 * m[3] + c2 * m[6]);
    const double invdet = 1.0 / det;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[i * 3 + j] = cof(j, i) * invdet;
}

// _transform_cam_to_lidar = transform_lidar_to_cam.inverse()   (DepthEstimator.cpp:44), as mld_create forms it
inline void camera_to_lidar(const double T[12], double Tinv[12]) {
    const double Lm[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    double Li[9];
    inverse3(Lm, Li);
    const double t[3] = {T[3], T[7], T[11]};
    for (int i = 0; i < 3; i++) {
        Tinv[i * 4 + 0] = Li[i * 3 + 0];
        Tinv[i * 4 + 1] = Li[i * 3 + 1];
        Tinv[i * 4 + 2] = Li[i * 3 + 2];
        Tinv[i * 4 + 3] = (-Li[i * 3 + 0]) * t[0] + ((-Li[i * 3 + 1]) * t[1] + (-Li[i * 3 + 2]) * t[2]);
    }
}

// The half sizes of the narrow (1) and the wide (2) window: NeighborFinderPixel.cpp:67-68, scales (1, 1) and (2.0f, 1.5f)
// (DepthEstimator.cpp:509,585)
inline void window_halves(const mld_params& P, double& halfX1, double& halfY1, double& halfX2, double& halfY2) {
    halfX1 = (double)P.pixelarea_search_witdh * 0.5 * (double)1.0f;
    halfY1 = (double)P.pixelarea_search_height * 0.5 * (double)1.0f;
    halfX2 = (double)P.pixelarea_search_witdh * 0.5 * (double)2.0f;
    halfY2 = (double)P.pixelarea_search_height * 0.5 * (double)1.5f;
}

// Upper bound on the columns / rows a window of this half size spans: floor(2 half) + 2, and no more than the image has.
inline int window_span(double half, int size) {
    const double n = std::floor(2.0 * half) + 2.0;
    return n > (double)size ? size : (int)n;
}
// Upper bound on the cells a window can cover.
inline double window_cells(double halfX, double halfY, int W, int H) {
    double nx = std::floor(2.0 * halfX) + 2.0, ny = std::floor(2.0 * halfY) + 2.0;
    if (nx > (double)W) nx = (double)W;
    if (ny > (double)H) ny = (double)H;
    return nx * ny;
}

inline void build_calib(DepthCalib& c, const mld_params& P, const mld_camera& cam, const double T[12]) {
    camera_to_lidar(T, c.Tinv);
    const double K[9] = {cam.focal_length, 0, cam.principal_point_x, 0, cam.focal_length, cam.principal_point_y, 0, 0, 1};
    inverse3(K, c.Kinv);
    c.W = cam.width;
    c.H = cam.height;
    window_halves(P, c.halfX1, c.halfY1, c.halfX2, c.halfY2);
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

// What mld_create refuses, with its texts, in its order; every function returns MLD_OK or the code and the text in `why`.
// A unit calls them in the order it documents, between what only it refuses.
inline int refuse_modes(const mld_params& P, std::string& why) {
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
    return MLD_OK;
}
inline int refuse_window_and_image(const mld_params& P, const mld_camera& cam, std::string& why) {
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
    return MLD_OK;
}
inline int refuse_intrinsics(const mld_camera& cam, std::string& why) {
    if (!std::isfinite(cam.focal_length) || cam.focal_length == 0.0 || !std::isfinite(cam.principal_point_x) ||
        !std::isfinite(cam.principal_point_y)) {
        why = "bad camera intrinsics";
        return MLD_ERR_INVALID_ARG;
    }
    return MLD_OK;
}
inline int refuse_transform(const double T[12], std::string& why) {
    for (int t = 0; t < 12; t++)
        if (!std::isfinite(T[t])) {
            why = "non-finite lidar->camera transform";
            return MLD_ERR_INVALID_ARG;
        }
    return MLD_OK;
}
// What the users of the lists refuse on top: a wide window of more than kMaxCells cells.
inline int refuse_wide_window_cells(const mld_params& P, const mld_camera& cam, std::string& why) {
    double halfX1, halfY1, halfX2, halfY2;
    window_halves(P, halfX1, halfY1, halfX2, halfY2);
    if (window_cells(halfX2, halfY2, cam.width, cam.height) > (double)kMaxCells) {
        why = "the wide window (2.0 x 1.5 the search area) can cover more than 1024 cells";
        return MLD_ERR_CAPACITY;
    }
    return MLD_OK;
}

// What the collect calls of the per-feature units refuse alike of the feature tables (u = uv and v null, or kTracks: u, v)
// and of the tables of the exported clouds, one entry per sequence each: every function returns the text of the first fault
// or null.  In their order; a unit puts what only it refuses (its record table, its bounds, its lists) between and behind
// them.  All are MLD_ERR_INVALID_ARG but feature_capacity_fault: MLD_ERR_CAPACITY.
struct FeatureTables {
    const void* const* u;
    const float* const* v;
    const int64_t* n_features;
    const int32_t* const* map;
    const int32_t* const* index;
    const int64_t* index_len;
    const double* const* cam;
    const int64_t* n_points;
};
template <bool kTracks>
inline const char* feature_table_fault(const FeatureTables& t) {
    if (!t.u) return kTracks ? "null table u" : "null table uv";
    if (kTracks && !t.v) return "null table v";
    if (!t.n_features) return "null table n_features";
    if (!t.map) return "null table map";
    if (!t.index) return "null table index";
    if (!t.index_len) return "null table index_len";
    if (!t.cam) return "null table cam";
    if (!t.n_points) return "null table n_points";
    return nullptr;
}
// Sequence s: its counts,
inline const char* feature_sign_fault(const FeatureTables& t, int s) {
    if (t.n_features[s] < 0) return "negative n_features";
    if (t.index_len[s] < 0) return "negative index_len";
    if (t.n_points[s] < 0) return "negative n_points";
    return nullptr;
}
inline const char* feature_capacity_fault(const FeatureTables& t, int s, int64_t max_features) {
    if (t.n_features[s] > max_features) return "n_features exceeds the max_features of the object";
    if (t.n_points[s] > kMaxPoints || t.index_len[s] > kMaxPoints) return "n_points or index_len exceeds 8 388 607";
    return nullptr;
}
// and, when it has features, its arrays: there (a unit tests its record array behind these), then aligned.
template <bool kTracks>
inline const char* feature_array_fault(const FeatureTables& t, int s) {
    if (!t.u[s]) return kTracks ? "null array u of a sequence with features" : "null array uv of a sequence with features";
    if (kTracks && !t.v[s]) return "null array v of a sequence with features";
    if (!t.map[s]) return "null array map of a sequence with features";
    if (t.index_len[s] > 0 && !t.index[s]) return "null array index of a sequence with features and index_len > 0";
    if (t.n_points[s] > 0 && !t.cam[s]) return "null array cam of a sequence with features and n_points > 0";
    return nullptr;
}
template <bool kTracks>
inline const char* feature_alignment_fault(const FeatureTables& t, int s) {
    auto off = [](const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (kTracks && off(t.u[s], 3u)) return "u must be 4-byte aligned";
    if (kTracks && off(t.v[s], 3u)) return "v must be 4-byte aligned";
    if (!kTracks && off(t.u[s], 7u)) return "uv must be 8-byte aligned";
    if (off(t.map[s], 3u)) return "map must be 4-byte aligned";
    if (off(t.index[s], 3u)) return "index must be 4-byte aligned";
    if (off(t.cam[s], 7u)) return "cam must be 8-byte aligned";
    return nullptr;
}

// The grid of a per-feature kernel for n_seq sequences, the longest of `longest` features; false: no feature, nothing to
// launch.
inline bool feature_grid(int n_seq, int64_t longest, dim3& grid) {
    grid = dim3((unsigned)n_seq, (unsigned)(longest < kMaxGridY ? longest : kMaxGridY));
    return longest > 0;
}

}  // namespace mld_batch
