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
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, V3, the wavefront helpers and the
// size limits: ../batch/mld_batch_device.h).  The records are nevertheless bit for bit what that path and the CPU
// restatement compute (tests/test_feature_traces_gpu.py pins that): the stages B2 to B6 are the functions of
// ../batch/mld_depth_path.h, the batch units' one restatement, operation for operation, of that path's arithmetic
// (gather_window, hist_segment, max_spanning_triangle, finish_main with plane_through, viewing_ray, intersect and the
// thresholds, far_from_plane; Tinv and Kinv formed as mld_create forms them), and this unit is compiled without contraction
// like the rest of the library.  What stands here is what only the trace has: the lists it keeps, the road states, the
// record.
#include <hip/hip_runtime.h>

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

constexpr int kMaxGridY = 65535;       // features of a sequence beyond it share blocks (grid-stride)

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

// The lists of the feature a wavefront works on, c.cap entries each (dynamic LDS): the points (PointList::x, y, z) and
struct Lists : PointList {
    int32_t* vis;  // visible index of neighbour i
    int32_t* aux;  // the histogram's bin of neighbour i; in the road stage its original index
    int32_t* pos;  // positions of the segmented points in the neighbour list; in the road stage those of the inliers
};

// gather_window of the depth path's header; besides, the visible indices go into the list and into `row` (up to list_cap of
// them), or row is null.
__device__ __forceinline__ int gather_visible(const DepthCalib& c, const TrSeq& q, double u, double v, double halfX, double halfY,
                                             const Lists& L, int lane, MLD_BATCH_GLOBAL int32_t* row, int list_cap, bool& bad) {
    return gather_window(c, q, u, v, halfX, halfY, L, lane, bad, [&](int rank, int m, int orig) {
        L.vis[rank] = m;
        L.aux[rank] = orig;
        if (row && rank < list_cap) row[rank] = m;
    });
}

template <bool kTracks>
__device__ __forceinline__ void trace_feature(const DepthCalib& c, const TrSeq& q, const Lists& L, mld_feature_trace* rec,
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
    const int n_nb = gather_visible(c, q, u, v, c.halfX1, c.halfY1, L, lane, q.nb ? as_global(q.nb) + row : nullptr, list_cap, bad);
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
            ks = hist_segment(c, n_nb, L, L.aux, lane, lower, higher, [&](int rank, int i) { L.pos[rank] = i; });
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
                main_type = finish_main(c, u, v, c1, c2, c3, mn, mx, &pl, main_depth);
            }
        }
    }
    __syncthreads();  // (the lists are rewritten from here)

    // ---- the road fallback (:578-597): the wide window, the distance test, the mask ----
    int road_state = MLD_TRACE_ROAD_NOT_REACHED, n_road = 0, n_inl = 0;
    if (c.useRoad && q.mask && main_type != MLD_Success && main_type != MLD_RadiusSearchInsufficientPoints) {
        n_road = gather_visible(c, q, u, v, c.halfX2, c.halfY2, L, lane, q.road ? as_global(q.road) + row : nullptr, list_cap, bad);
        __syncthreads();
        if ((unsigned)n_road < c.countMin) {  // :585-586
            road_state = MLD_TRACE_ROAD_FEW_NEIGHBOURS;
        } else {
            // CalculateDepthSegmentationPlane (:782-900)
            bool anyFar = false;
            int kk = 0;
            for (int b = 0; b < n_road; b += kWave) {
                const int i = b + lane;
                bool far = false, inl = false;
                if (i < n_road) {
                    far = far_from_plane(c.Tinv, q.coeffs, c.roadDistThr, list_point(L, i));
                    inl = mask_bit(q.mask, L.aux[i]);
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
__global__ __launch_bounds__(kWave) void k_feature_trace(const TrSeq* __restrict__ desc, DepthCalib c, int list_cap) {
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

// What only this object refuses, first and last; between them what mld_create refuses of a parameter set, a camera and a
// transform, with its texts.
int refuse_config(const mld_params& P, const mld_camera& cam, const double T[12], std::string& why) {
    if (P.do_use_PCA) {
        why = "do_use_PCA: the eigen-solve is a tolerance path, the trace promises equality";
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

struct mld_feature_traces : mld_batch::Object {
    int n_seq = 0;
    int64_t max_features = 0;
    DepthCalib calib{};
    size_t lds_bytes = 0;
    mld_batch::DescRing<TrSeq> ring;
};

namespace {

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
    hipLaunchKernelGGL(k_feature_trace<kTracks>, dim3((unsigned)S, gy), dim3(kWave), ft->lds_bytes, ft->stream, ft->ring.d_desc.get(),
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
    std::string why;
    // (what is refused with a status of its own; still nothing of the context is used)
    const int code = bad ? MLD_OK : refuse_config(*params, *camera, T_cam_lidar, why);
    auto init = [&](mld_feature_traces* ft) {
        ft->n_seq = n_seq;
        ft->max_features = max_features;
        build_calib(ft->calib, *params, *camera, T_cam_lidar);
        ft->lds_bytes = (size_t)ft->calib.cap * 36 + sizeof(mld_feature_trace);
        return ft->ring.allocate(ft, n_seq);
    };
    return mld_batch::create_object<mld_feature_traces>(g_error, "mld_feature_traces_create", bad, ctx, status_out, init, code,
                                                        why.c_str());
}

void mld_feature_traces_destroy(mld_feature_traces* ft) { mld_batch::destroy_object(ft); }

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
