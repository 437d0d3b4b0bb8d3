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
//     B3 to B6  main_path of ../batch/mld_depth_path.h on that list: the count test; the histogram's bins from ballots
//         over the list, the scan for the first local maximum on the scalar side, the kept points compacted in place
//         (HistogramPointDepth.cpp:15-123); the farthest pair and the third corner by (value descending, id ascending)
//         reductions (PlaneEstimationCalcMaxSpanningTriangle.cpp:37-100); the serial tail - planarity, viewing ray,
//         Hyperplane::Through, intersection, thresholds - on wave-uniform values.  Its functor for the kept points also
//         writes the seg row; lane 0 stages the corners' visible indices and the record's doubles in LDS at once
//     road  the wide window as B2, then per neighbour the f32 point-to-plane distance after the f64 Tinv transform and the
//         mask bit of its original index (DepthEstimator.cpp:782-900); then the record's integers, and the record leaves
//         as one store of a dword per lane
// The road fit itself is not repeated: its depth is the depth path's business.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, V3, the wavefront helpers and the
// size limits: ../batch/mld_batch_device.h).  The records are nevertheless bit for bit what that path and the CPU
// restatement compute (tests/test_feature_traces_gpu.py pins that): the stages B2 to B6 are the functions of
// ../batch/mld_depth_path.h, the batch units' one restatement, operation for operation, of that path's arithmetic
// (gather_window, main_path, far_from_plane; Tinv and Kinv formed as mld_create forms them), and this unit is compiled
// without contraction like the rest of the library.  That header also has what this unit shares with the other unit of one
// wavefront per feature: the lists, the feature reader, the record's exit, the refusals of the collect calls they have in
// common and the grid.  What stands here is what only the trace has: the rows it keeps, the road states, the record
// (profiles/feature_units.md: what the move did to the kernel).
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

static_assert(sizeof(mld_feature_trace) == 184, "184 bytes per record (include/mld.h)");
static_assert(offsetof(mld_feature_trace, main_depth) == 56 && offsetof(mld_feature_trace, corners) == 112,
              "field offsets of the record (include/mld.h)");

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
    read_feature<kTracks>(q.u, q.v, f, u, v);
    const size_t row = (size_t)f * (size_t)list_cap;
    int flags = (isfinite(u) && isfinite(v)) ? 0 : MLD_TRACE_FLAG_NONFINITE_FEATURE;
    bool bad = false;

    // ---- B2: the narrow window (DepthEstimator.cpp:509, scale 1.0 x 1.0) ----
    const int n_nb = gather_visible(c, q, u, v, c.halfX1, c.halfY1, L, lane, q.nb ? as_global(q.nb) + row : nullptr, list_cap, bad);
    __syncthreads();
    // ---- B3 to B6: the main path on the window's list ----
    MLD_BATCH_GLOBAL int32_t* seg_row = q.seg ? as_global(q.seg) + row : nullptr;
    const MainPath mp = main_path(c, u, v, n_nb, L, L.aux, lane, [&](int rank, int i) {
        L.pos[rank] = i;
        if (seg_row && rank < list_cap) seg_row[rank] = i;
    });
    int cv0 = -1, cv1 = -1, cv2 = -1;  // (one uniform branch: the six LDS reads of the corners are in flight together)
    if (mp.ci >= 0) cv0 = L.vis[L.pos[mp.ci]], cv1 = L.vis[L.pos[mp.cj]], cv2 = L.vis[L.pos[mp.ck]];
    if (lane == 0) {  // staged while the lists hold the corners: what was read from them, and the doubles (the registers go)
        rec->corner_vis[0] = cv0, rec->corner_vis[1] = cv1, rec->corner_vis[2] = cv2;
        rec->main_depth = mp.depth;
        rec->hist_lower = mp.lower;
        rec->hist_higher = mp.higher;
        rec->plane_n[0] = mp.plane.n.x, rec->plane_n[1] = mp.plane.n.y, rec->plane_n[2] = mp.plane.n.z;
        rec->plane_offset = mp.plane.offset;
        rec->corners[0] = mp.c1.x, rec->corners[1] = mp.c1.y, rec->corners[2] = mp.c1.z;
        rec->corners[3] = mp.c2.x, rec->corners[4] = mp.c2.y, rec->corners[5] = mp.c2.z;
        rec->corners[6] = mp.c3.x, rec->corners[7] = mp.c3.y, rec->corners[8] = mp.c3.z;
    }
    __syncthreads();  // (the lists are rewritten from here)

    // ---- the road fallback (:578-597): the wide window, the distance test, the mask ----
    int road_state = MLD_TRACE_ROAD_NOT_REACHED, n_road = 0, n_inl = 0;
    if (c.useRoad && q.mask && mp.type != MLD_Success && mp.type != MLD_RadiusSearchInsufficientPoints) {
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

    // ---- the integers of the record; it leaves as one store of a dword per lane (profiles/feature_units.md: the forms) ----
    if (lane == 0) {
        rec->main_type = mp.type;
        rec->n_nb = n_nb;
        rec->n_seg = mp.n_seg;
        rec->corner_pos[0] = mp.ci, rec->corner_pos[1] = mp.cj, rec->corner_pos[2] = mp.ck;
        rec->road_state = road_state;
        rec->n_road = n_road;
        rec->n_road_inl = n_inl;
        rec->flags = flags;
        rec->pad_ = 0;
    }
    store_record(rec, q.trace + f, lane);
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
    auto bad_arg = [&](const char* text) { return refuse(MLD_ERR_INVALID_ARG, text); };
    const FeatureTables t = {u_tab, v_tab, n_features, map, index, index_len, cam, n_points};
    const char* bad;
    if ((bad = feature_table_fault<kTracks>(t))) return bad_arg(bad);
    if (!trace_out) return bad_arg("null table trace_out");
    if (list_capacity < 0 || list_capacity > kMaxCells) return bad_arg("list_capacity must be in 0 .. 1024");
    if ((coeffs != nullptr) != (mask_dev != nullptr)) return bad_arg("coeffs and mask_dev come together or not at all");
    const int S = ft->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if ((bad = feature_sign_fault(t, s))) return bad_arg(bad);
        if ((bad = feature_capacity_fault(t, s, ft->max_features))) return refuse(MLD_ERR_CAPACITY, bad);
        const int64_t n = n_features[s];
        if (n == 0) continue;  // (needs no arrays)
        if ((bad = feature_array_fault<kTracks>(t, s))) return bad_arg(bad);
        if (!trace_out[s]) return bad_arg("null array trace_out of a sequence with features");
        if ((bad = feature_alignment_fault<kTracks>(t, s))) return bad_arg(bad);
        if (mask_dev && misaligned(mask_dev[s], 3u)) return bad_arg("mask_dev must be 4-byte aligned");
        if (misaligned(trace_out[s], 7u)) return bad_arg("trace_out must be 8-byte aligned");
        if (list_capacity > 0) {
            if (nb_out && misaligned(nb_out[s], 3u)) return bad_arg("nb_out must be 4-byte aligned");
            if (seg_out && misaligned(seg_out[s], 3u)) return bad_arg("seg_out must be 4-byte aligned");
            if (road_out && misaligned(road_out[s], 3u)) return bad_arg("road_out must be 4-byte aligned");
            if (road_inl_out && misaligned(road_inl_out[s], 3u)) return bad_arg("road_inl_out must be 4-byte aligned");
        }
        if (n > longest) longest = n;
    }
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
    dim3 grid;
    if (!feature_grid(S, longest, grid)) return MLD_OK;
    MLD_HIP(ft, hipSetDevice(ft->device));
    const int rc = ft->ring.upload(ft);
    if (rc) return rc;
    hipLaunchKernelGGL(k_feature_trace<kTracks>, grid, dim3(kWave), ft->lds_bytes, ft->stream, ft->ring.d_desc.get(), ft->calib,
                       list_capacity);
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
