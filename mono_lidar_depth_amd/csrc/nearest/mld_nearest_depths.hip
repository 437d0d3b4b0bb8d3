// mld_nearest_depths.hip — the main path on the k closest returns of a feature, for a batch of sequences in one call
// (include/mld.h, "mld_nearest_depths"): the neighbour search the reference designed as neighbor_search_mode 1
// (parameters.yaml:5, NeighborFinderKdd: nnSearch_count nearest, or all within radiusSearch_radius) and never finished,
// as an exact search over the cells of the pixel map.  A feature whose fixed rectangle holds too few returns
// (RadiusSearchInsufficientPoints) gets a list that follows the local density of the returns instead.  The inputs are the
// arrays mld_projected_clouds_export_device writes (pixel map, _pointIndex, camera-frame cloud).  No frame slot is
// involved, nothing is allocated per call, nothing comes back to the host, no global atomics, no floating-point
// accumulation.
//
// Two launches: the descriptor upload and
//   k_nearest_depths   grid (sequence, feature), ONE WAVEFRONT PER FEATURE, radius R <= 64, count k <= 256:
//     N1  the disc around the centre cell in square stages of half size 4, 8, 16, 32, 64 (capped at R), each stage only its
//         new cells, row-major, 64 cells per step (the rows of a stage are contiguous: the loads coalesce along x), four
//         steps' loads in flight, the row and column of a lane's cell stepped without a division per cell.  Every
//         candidate is counted (n_in_radius, BAD_INPUT are about the whole disc); while the search is open its d2 also
//         goes into a histogram in LDS, one BYTE per distance (at most 32 cells share a d2 <= 4096), by ds_add on the word.
//     N2  after a stage of half size r every cell with d2 <= r * r has been seen: when k candidates lie within that
//         circle, or at r >= R, the search is over and the later stages only count.  (k candidates SEEN is not the
//         condition: the corner (3, 3) of a stage, d2 18, is farther than the axis cell (4, 0) of the next one.  The
//         histogram keeps the corners' candidates until their circle is complete.)
//     N3  the cut-off distance D - the smallest with k candidates at or below it - from a prefix scan over the
//         histogram's new bins; the candidates with d2 <= D (at most k + 31) gathered from the disc of radius sqrt(D),
//         which the caches still hold; each ranked by counting the smaller keys (d2, y, x) among them: its rank is its
//         place in the list, the ranks at and beyond k fall away.  No comparison sort, no order left to the hardware.
//     N4  the list's points through main_path of ../batch/mld_depth_path.h (count test, histogram segmentation, corners,
//         B6) with the viewing ray through the exact (u, v); the record is staged in LDS by lane 0 and leaves as one store
//         of a dword per lane.
//
// Per block (one wavefront), from the compiler's resource report for gfx950 (-Rpass-analysis=kernel-resource-usage):
//   LDS       dynamic, 40 (k + k % 2) + 12 (k + 32) + 4 (R * R / 4 + 1) + 64 bytes: 1 072 at (R, k) = (10, 10), 1 860 at
//             (24, 16), 15 364 at (40, 256), 17 860 at (64, 256)
//   VGPRs     110 (both instantiations), 106 SGPRs; SGPR spills go to VGPR lanes
//   scratch   0
//   wavefronts per CU   16 by registers (4 per SIMD); by LDS (160 KiB per CU) that many up to 10 KiB per block, 10 at
//             (40, 256) and 9 at (64, 256)
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring and object skeleton: ../batch/mld_batch_object.h; as_global, V3, the wavefront helpers and the
// size limits: ../batch/mld_batch_device.h; the main path, the calibration, the refusals it shares with mld_create, and
// what it shares with the feature traces, the other unit of one wavefront per feature - the lists, the feature reader, the
// record's exit, the common refusals of the collect calls, the grid: ../batch/mld_depth_path.h).  It is compiled without contraction like the rest of the library; the records are bit for
// bit what the CPU restatement computes (tests/test_nearest_depths_gpu.py pins that).
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

constexpr int kFirstStage = 4;    // half size of the first square
constexpr int kInFlight = 4;     // steps of 64 cells whose loads a wavefront has in flight
constexpr int kTieRoom = 32;      // cells that can share one d2 <= 4096 (1105 = 5 * 13 * 17 has 32 lattice points)

static_assert(sizeof(mld_nearest_depth) == 64, "64 bytes per record (include/mld.h)");
static_assert(offsetof(mld_nearest_depth, depth) == 32 && offsetof(mld_nearest_depth, nearest_z) == 40 &&
                  offsetof(mld_nearest_depth, corner_vis) == 48 && alignof(mld_nearest_depth) == 8,
              "field offsets of the record (include/mld.h)");
static_assert(MLD_NEAREST_MAX_RADIUS == 64 && MLD_NEAREST_MAX_COUNT == 256, "the stages, the keys and the LDS budget assume them");

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct NdSeq {
    const void* u;         // uv, 2 x n_feat f64 (collect_device); u, n_feat f32 (collect_tracks_device)
    const float* v;        // tracks form only
    const int32_t* map;    // W * H: visible index or -1
    const int32_t* index;  // index_len: original index of a visible point
    const double* cam;     // 3 x n_points
    mld_nearest_depth* rec;
    int32_t* nb;           // list_capacity x n_feat, or null
    int32_t n_feat;
    int32_t index_len;
    int32_t n_points;
    int32_t pad_;
};
static_assert(sizeof(NdSeq) == 72, "72 bytes per sequence (include/mld.h, DESIGN.md)");

// What a wavefront keeps of its feature (dynamic LDS) beside the lists of the depth path's header (x, y, z, vis, aux, pos: k2
// entries each, k2 = k rounded up to even; aux[0] is the original index of the first entry until the bins overwrite it).
struct NearestLists : Lists {
    uint32_t* skey;  // k2: key of list entry i
    uint32_t* ckey;  // k + kTieRoom: keys of the gathered candidates, d2 << 16 | (dy + 64) << 8 | (dx + 64)
    int32_t* cm;     // their visible indices
    int32_t* co;     // their original indices
    uint32_t* hist;  // R * R / 4 + 1 words: candidates at distance d2 in byte d2
};

// The map value of a cell as a candidate: its visible index m and original index o, or nothing (a value outside the
// arrays: nothing, and `bad`).
__device__ __forceinline__ bool candidate(const NdSeq& q, const MLD_BATCH_GLOBAL int32_t* index, int m, int& o, bool& bad) {
    if (m == -1) return false;
    if (m < 0 || m >= q.index_len) {
        bad = true;
        return false;
    }
    o = index[m];
    if (o < 0 || o >= q.n_points) {
        bad = true;
        return false;
    }
    return true;
}

// The clipped square of half size r around (cx, cy): false when it holds no cell of the image.
__device__ __forceinline__ bool clip_square(const DepthCalib& c, int cx, int cy, int r, int& x0, int& y0, int& nx, int& ncell) {
    x0 = max(cx - r, 0);
    y0 = max(cy - r, 0);
    nx = min(cx + r, c.W - 1) - x0 + 1;
    const int ny = min(cy + r, c.H - 1) - y0 + 1;
    ncell = nx * ny;  // (at most 129 x 129)
    return nx > 0 && ny > 0;
}

// N1 to N3 for the centre cell (cx, cy): the list in L (points, vis, skey; aux[0]), its length; n_in: the candidates of the
// whole disc.  Every lane is here.
__device__ __forceinline__ int nearest_list(const DepthCalib& c, const NdSeq& q, const NearestLists& L, const int cx, const int cy,
                                            const int R, const int K, const int lane, MLD_BATCH_GLOBAL int32_t* row, const int list_cap,
                                            int& n_in, bool& bad) {
    const MLD_BATCH_GLOBAL int32_t* map = as_global(q.map);
    const MLD_BATCH_GLOBAL int32_t* index = as_global(q.index);
    const MLD_BATCH_GLOBAL double* cam = as_global(q.cam);
    const unsigned char* histb = reinterpret_cast<const unsigned char*>(L.hist);
    const int R2 = R * R;
    bool badl = false;
    int total = 0;       // candidates counted so far
    int cum = 0;         // while the search is open: candidates with d2 <= p * p
    int p = -1;          // half size of the square behind us
    int words = 0;       // words of the histogram zeroed so far
    bool open = true;    // the search; closed: the stages only count
    int lo = 0, hi = -1, at_hi = 0;  // when the search closed: the bins (lo .. hi] were new, at_hi candidates up to hi
    for (int r = min(kFirstStage, R);; r = min(2 * r, R)) {  // (uniform)
        if (open) {  // the bins this stage can reach: d2 <= 2 r * r, in the disc
            const int need = (min(2 * r * r, R2) >> 2) + 1;
            for (int w = words + lane; w < need; w += kWave) L.hist[w] = 0u;
            words = need;
            __syncthreads();
        }
        int x0, y0, nx, ncell;
        if (clip_square(c, cx, cy, r, x0, y0, nx, ncell)) {
            // kInFlight steps at a time, their loads issued in stages - the map values, then the indices of the occupied
            // cells - so that a wavefront waits for two loads per 256 cells and not per 64
            // (row, column) of a lane's cell without a division per cell: 64 cells on are step_r rows and step_c columns on
            const int step_r = uniform(kWave / nx), step_c = kWave - step_r * nx;
            int rr = lane / nx, col = lane - rr * nx;
            for (int base = 0; base < ncell; base += kInFlight * kWave) {
                int m[kInFlight], d2[kInFlight], o[kInFlight];
                bool filled[kInFlight];
#pragma unroll
                for (int j = 0; j < kInFlight; j++) {
                    const int cidx = base + j * kWave + lane;
                    const int dx = x0 + col - cx, dy = y0 + rr - cy;
                    d2[j] = dx * dx + dy * dy;
                    m[j] = -1;
                    if (cidx < ncell && d2[j] <= R2 && max(abs(dx), abs(dy)) > p)
                        m[j] = map[(size_t)(x0 + col) + (size_t)(y0 + rr) * (size_t)c.W];
                    col += step_c;
                    rr += step_r;
                    if (col >= nx) {
                        col -= nx;
                        rr++;
                    }
                }
#pragma unroll
                for (int j = 0; j < kInFlight; j++) {
                    filled[j] = m[j] != -1;
                    o[j] = -1;
                    if (filled[j] && m[j] >= 0 && m[j] < q.index_len) o[j] = index[m[j]];
                }
#pragma unroll
                for (int j = 0; j < kInFlight; j++) {
                    const bool has = filled[j] && o[j] >= 0 && o[j] < q.n_points;  // (a map value outside the index left o at -1)
                    if (filled[j] && !has) badl = true;
                    total += (int)__popcll(__ballot(has));
                    if (open && has) atomicAdd(&L.hist[d2[j] >> 2], 1u << ((d2[j] & 3) * 8));
                }
            }
        }
        if (open) {  // N2
            __syncthreads();
            const int from = p < 0 ? 0 : p * p + 1, to = min(r * r, R2);
            int s = 0;
            for (int b = from + lane; b <= to; b += kWave) s += (int)histb[b];
            const int inside = cum + wave_sum(s);
            if (inside >= K || r >= R) {
                open = false;
                lo = from, hi = to, at_hi = inside;
            } else {
                cum = inside;
            }
        }
        if (r >= R) break;
        p = r;
    }
    n_in = uniform(total);
    at_hi = uniform(at_hi);
    if (__ballot(badl) != 0ull) bad = true;
    if (at_hi == 0) return 0;

    // ---- N3: the cut-off distance D and the candidates up to it
    int D = hi, n_le = at_hi;  // fewer than K in the disc: all of them
    if (at_hi >= K) {
        int ahead = uniform(cum);  // candidates below bin `lo`: fewer than K
        for (int b0 = lo; b0 <= hi; b0 += kWave) {
            const int b = b0 + lane;
            const int incl = ahead + scan_inclusive<kWave>(b <= hi ? (int)histb[b] : 0, lane);
            const unsigned long long reach = __ballot(incl >= K);
            if (reach != 0ull) {
                const int first = (int)__ffsll((long long)reach) - 1;
                D = b0 + first;
                n_le = __shfl(incl, first);
                break;
            }
            ahead = __shfl(incl, kWave - 1);
        }
        D = uniform(D);
        n_le = uniform(n_le);
    }
    int s = (int)sqrtf((float)D);  // floor(sqrt(D))
    while (s * s > D) s--;
    while ((s + 1) * (s + 1) <= D) s++;
    const int room = K + kTieRoom;
    int ncand = 0;
    int x0, y0, nx, ncell;
    if (clip_square(c, cx, cy, s, x0, y0, nx, ncell)) {
        for (int base = 0; base < ncell; base += kWave) {
            const int cidx = base + lane;
            const int rr = cidx / nx, col = cidx - rr * nx;
            const int x = x0 + col, y = y0 + rr;
            const int dx = x - cx, dy = y - cy;
            const int d2 = dx * dx + dy * dy;
            int m = -1, o = 0;
            if (cidx < ncell && d2 <= D) m = map[(size_t)x + (size_t)y * (size_t)c.W];
            bool again = false;
            const bool has = candidate(q, index, m, o, again);
            const unsigned long long mk = __ballot(has);
            const int at = ncand + prefix_count(mk);
            if (has && at < room) {
                L.ckey[at] = ((unsigned)d2 << 16) | ((unsigned)(dy + 64) << 8) | (unsigned)(dx + 64);
                L.cm[at] = m;
                L.co[at] = o;
            }
            ncand += (int)__popcll(mk);
        }
    }
    ncand = uniform(min(min(ncand, n_le), room));  // (== n_le <= K + 31; the bounds are for the memory's sake)
    __syncthreads();
    // the rank of a candidate: the smaller keys among them (the keys differ: a cell has one)
    for (int i = lane; i < ncand; i += kWave) {
        const unsigned key = L.ckey[i];
        int rank = 0;
        for (int j = 0; j < ncand; j++) rank += (L.ckey[j] < key) ? 1 : 0;
        if (rank < K) {
            const int m = L.cm[i], o = L.co[i];
            L.skey[rank] = key;
            L.vis[rank] = m;
            L.x[rank] = cam[3 * (size_t)o];
            L.y[rank] = cam[3 * (size_t)o + 1];
            L.z[rank] = cam[3 * (size_t)o + 2];
            if (rank == 0) L.aux[0] = o;
            if (row && rank < list_cap) row[rank] = m;
        }
    }
    __syncthreads();
    return min(ncand, K);
}

template <bool kTracks>
__device__ __forceinline__ void nearest_feature(const DepthCalib& c, const NdSeq& q, const NearestLists& L, mld_nearest_depth* rec,
                                                const int f, const int lane, const int R, const int K, const int list_cap) {
    double u, v;
    read_feature<kTracks>(q.u, q.v, f, u, v);
    const bool finite = isfinite(u) && isfinite(v);
    int flags = finite ? 0 : MLD_NEAREST_FLAG_NONFINITE_FEATURE;
    bool bad = false;
    int n_in = 0, n_nb = 0;
    if (__ballot(finite) != 0ull) {  // (uniform: every lane read the same feature)
        // the clamp in f64 ahead of the cast: no cast is undefined, a feature far outside has an empty disc
        const double ux = fmin(fmax(u, -(double)(R + 1)), (double)(c.W + R));
        const double vy = fmin(fmax(v, -(double)(R + 1)), (double)(c.H + R));
        const int cx = uniform((int)floor(ux)), cy = uniform((int)floor(vy));
        n_nb = nearest_list(c, q, L, cx, cy, R, K, lane, q.nb ? as_global(q.nb) + (size_t)f * (size_t)list_cap : nullptr, list_cap,
                            n_in, bad);
    }
    int d2_first = -1, d2_last = -1, nearest_orig = -1;
    double nearest_z = __builtin_nan("");
    if (n_nb > 0) {  // (read before the segmentation compacts the list and the bins overwrite aux)
        d2_first = (int)(L.skey[0] >> 16);
        d2_last = (int)(L.skey[n_nb - 1] >> 16);
        nearest_orig = L.aux[0];
        nearest_z = L.z[0];
    }
    __syncthreads();
    const MainPath mp = main_path(c, u, v, n_nb, L, L.aux, lane, [&](int rank, int i) { L.pos[rank] = i; });
    if (bad) flags |= MLD_NEAREST_FLAG_BAD_INPUT;

    // ---- the record: staged by lane 0, stored as one dword per lane ----
    if (lane == 0) {
        rec->type = mp.type;
        rec->n_in_radius = n_in;
        rec->n_nb = n_nb;
        rec->n_seg = mp.n_seg;
        rec->d2_first = d2_first;
        rec->d2_last = d2_last;
        rec->nearest_orig = nearest_orig;
        rec->flags = flags;
        rec->depth = mp.depth;
        rec->nearest_z = nearest_z;
        rec->corner_vis[0] = mp.ci >= 0 ? L.vis[L.pos[mp.ci]] : -1;
        rec->corner_vis[1] = mp.ci >= 0 ? L.vis[L.pos[mp.cj]] : -1;
        rec->corner_vis[2] = mp.ci >= 0 ? L.vis[L.pos[mp.ck]] : -1;
        rec->pad_ = 0;
    }
    store_record(rec, q.rec + f, lane);
}

// Bytes of dynamic LDS for count K and radius R, and the carving of them (the doubles first, the staged record behind
// them, then the 32-bit arrays).
__host__ __device__ inline int even_count(int K) { return (K + 1) & ~1; }
inline size_t lds_bytes_for(int R, int K) {
    return (size_t)even_count(K) * 40 + (size_t)(K + kTieRoom) * 12 + (size_t)(R * R / 4 + 1) * 4 + sizeof(mld_nearest_depth);
}

// Grid (sequence, feature); one wavefront per block.
template <bool kTracks>
__global__ __launch_bounds__(kWave) void k_nearest_depths(const NdSeq* __restrict__ desc, DepthCalib c, int R, int K, int list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const NdSeq q = desc[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int k2 = even_count(K), room = K + kTieRoom;
    NearestLists L;
    L.x = reinterpret_cast<double*>(smem);
    L.y = L.x + k2;
    L.z = L.y + k2;
    mld_nearest_depth* rec = reinterpret_cast<mld_nearest_depth*>(L.z + k2);
    L.vis = reinterpret_cast<int32_t*>(rec + 1);
    L.aux = L.vis + k2;
    L.pos = L.aux + k2;
    L.skey = reinterpret_cast<uint32_t*>(L.pos + k2);
    L.ckey = L.skey + k2;
    L.cm = reinterpret_cast<int32_t*>(L.ckey + room);
    L.co = L.cm + room;
    L.hist = reinterpret_cast<uint32_t*>(L.co + room);
    for (int f = (int)blockIdx.y; f < q.n_feat; f += (int)gridDim.y)  // (uniform in the block)
        nearest_feature<kTracks>(c, q, L, rec, f, lane, R, K, list_cap);
}

char g_error[512] = "";  // refusals without an object: mld_nearest_depths_last_error(NULL)

// What only this object refuses, first; then what mld_create refuses of a parameter set and a camera, with its texts.
int refuse_config(const mld_params& P, const mld_camera& cam, std::string& why) {
    if (P.do_use_PCA) {
        why = "do_use_PCA: the eigen-solve is a tolerance path, the records promise equality";
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    if (P.set_all_depths_to_zero) {
        why = "set_all_depths_to_zero: every depth is 0 there, the depth calls answer that without a kernel";
        return MLD_ERR_UNSUPPORTED_MODE;
    }
    int code = refuse_modes(P, why);
    if (code == MLD_OK) code = refuse_window_and_image(P, cam, why);
    if (code == MLD_OK) code = refuse_intrinsics(cam, why);
    return code;
}

}  // namespace

struct mld_nearest_depths : mld_batch::Object {
    int n_seq = 0;
    int64_t max_features = 0;
    int radius = 0, count = 0;
    DepthCalib calib{};
    size_t lds_bytes = 0;
    mld_batch::DescRing<NdSeq> ring;
};

namespace {

// Both collect calls: u_tab = uv (v_tab null) or u, v.
template <bool kTracks>
int collect(mld_nearest_depths* nd, const char* fn, const void* const* u_tab, const float* const* v_tab, const int64_t* n_features,
            const int32_t* const* map, const int32_t* const* index, const int64_t* index_len, const double* const* cam,
            const int64_t* n_points, int list_capacity, mld_nearest_depth* const* record_out, int32_t* const* nb_out) {
    if (!nd) return no_object(g_error, fn, "nd");
    auto refuse = [&](int code, const char* text) { return fail(nd, code, (std::string(fn) + ": " + text).c_str()); };
    auto bad_arg = [&](const char* text) { return refuse(MLD_ERR_INVALID_ARG, text); };
    const FeatureTables t = {u_tab, v_tab, n_features, map, index, index_len, cam, n_points};
    const char* bad;
    if ((bad = feature_table_fault<kTracks>(t))) return bad_arg(bad);
    if (!record_out) return bad_arg("null table record_out");
    if (list_capacity < 0 || list_capacity > nd->count) return bad_arg("list_capacity must be in 0 .. count");
    const int S = nd->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if ((bad = feature_sign_fault(t, s))) return bad_arg(bad);
        if ((bad = feature_capacity_fault(t, s, nd->max_features))) return refuse(MLD_ERR_CAPACITY, bad);
        const int64_t n = n_features[s];
        if (n == 0) continue;  // (needs no arrays)
        if ((bad = feature_array_fault<kTracks>(t, s))) return bad_arg(bad);
        if (!record_out[s]) return bad_arg("null array record_out of a sequence with features");
        if ((bad = feature_alignment_fault<kTracks>(t, s))) return bad_arg(bad);
        if (misaligned(record_out[s], 7u)) return bad_arg("record_out must be 8-byte aligned");
        if (list_capacity > 0 && nb_out && misaligned(nb_out[s], 3u)) return bad_arg("nb_out must be 4-byte aligned");
        if (n > longest) longest = n;
    }
    for (int s = 0; s < S; s++) {
        NdSeq& q = nd->ring.stage[(size_t)s];
        q = NdSeq{};
        const int64_t n = n_features[s];
        if (n == 0) continue;
        q.u = u_tab[s];
        q.v = kTracks ? v_tab[s] : nullptr;
        q.map = map[s];
        q.index = index[s];
        q.cam = cam[s];
        q.rec = record_out[s];
        q.nb = (list_capacity > 0 && nb_out) ? nb_out[s] : nullptr;
        q.n_feat = (int32_t)n;
        q.index_len = (int32_t)index_len[s];
        q.n_points = (int32_t)n_points[s];
    }
    dim3 grid;
    if (!feature_grid(S, longest, grid)) return MLD_OK;
    MLD_HIP(nd, hipSetDevice(nd->device));
    const int rc = nd->ring.upload(nd);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nearest_depths<kTracks>, grid, dim3(kWave), nd->lds_bytes, nd->stream, nd->ring.d_desc.get(), nd->calib,
                       nd->radius, nd->count, list_capacity);
    MLD_HIP(nd, hipGetLastError());
    return MLD_OK;
}

}  // namespace

extern "C" {

mld_nearest_depths* mld_nearest_depths_create(mld_ctx* ctx, int n_seq, int64_t max_features, int radius, int count,
                                              const mld_params* params, const mld_camera* camera, int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_nearest_depths_create: n_seq must be in 1 .. 65536";
        if (max_features < 1 || max_features > kMaxFeatures) return "mld_nearest_depths_create: max_features must be in 1 .. 16777216";
        if (radius < 1 || radius > MLD_NEAREST_MAX_RADIUS) return "mld_nearest_depths_create: radius must be in 1 .. 64";
        if (count < 1 || count > MLD_NEAREST_MAX_COUNT) return "mld_nearest_depths_create: count must be in 1 .. 256";
        if (!ctx) return "mld_nearest_depths_create: null context";
        if (!params) return "mld_nearest_depths_create: null params";
        if (!camera) return "mld_nearest_depths_create: null camera";
        return nullptr;
    };
    const char* bad = refusal();
    std::string why;
    // (what is refused with a status of its own; still nothing of the context is used)
    const int code = bad ? MLD_OK : refuse_config(*params, *camera, why);
    auto init = [&](mld_nearest_depths* nd) {
        nd->n_seq = n_seq;
        nd->max_features = max_features;
        nd->radius = radius;
        nd->count = count;
        const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // (nothing here reads Tinv)
        build_calib(nd->calib, *params, *camera, identity);
        nd->lds_bytes = lds_bytes_for(radius, count);
        return nd->ring.allocate(nd, n_seq);
    };
    return mld_batch::create_object<mld_nearest_depths>(g_error, "mld_nearest_depths_create", bad, ctx, status_out, init, code,
                                                        why.c_str());
}

void mld_nearest_depths_destroy(mld_nearest_depths* nd) { mld_batch::destroy_object(nd); }

const char* mld_nearest_depths_last_error(const mld_nearest_depths* nd) { return nd ? nd->err.c_str() : g_error; }

int mld_nearest_depths_collect_device(mld_nearest_depths* nd, const double* const* uv, const int64_t* n_features,
                                      const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                      const double* const* cam, const int64_t* n_points, int list_capacity,
                                      mld_nearest_depth* const* record_out, int32_t* const* nb_out) {
    return collect<false>(nd, "mld_nearest_depths_collect_device", reinterpret_cast<const void* const*>(uv), nullptr, n_features, map,
                          index, index_len, cam, n_points, list_capacity, record_out, nb_out);
}

int mld_nearest_depths_collect_tracks_device(mld_nearest_depths* nd, const float* const* u, const float* const* v,
                                             const int64_t* n_features, const int32_t* const* map, const int32_t* const* index,
                                             const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                             int list_capacity, mld_nearest_depth* const* record_out, int32_t* const* nb_out) {
    return collect<true>(nd, "mld_nearest_depths_collect_tracks_device", reinterpret_cast<const void* const*>(u), v, n_features, map,
                         index, index_len, cam, n_points, list_capacity, record_out, nb_out);
}

}  // extern "C"
