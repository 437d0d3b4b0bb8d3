// mld_ransac_planes.hip — RansacPlane::CalculateInliersPlane (monolidar_fusion/src/RansacPlane.cpp:41-140) for a batch
// of sequences in one call (include/mld.h, "mld_ransac_planes"): the plane of a frame that comes WITHOUT a label image,
// which DepthEstimator::setInputCloud estimates by default (DepthEstimator.cpp:275-283).  The twin of
// mld_semantic_planes.hip: no frame slot is involved, clouds are read where they lie, and the masks it writes are the
// mask_dev[s] arrays of mld_set_clouds_planes_range_device.
//
// Up to three launches, ordered by kernel boundaries alone (no flags, no waiting between blocks):
//   k_rp_pass      (z pass-through only) grid (sequence, 1024 points): pcl::PassThrough (:57-64) as one 64-bit candidate
//                  mask per 64 points and one count per 1024 points, both in the object's device scratch - whatever the
//                  size of the cloud, no table of the pass-through is held in LDS
//   k_rp_scan      (z pass-through only) one block per sequence: exclusive prefix of the counts, in place
//   k_rp_estimate  one block of 512 threads per sequence: clears the mask; stratified sample (:66-74) gathered into LDS;
//                  hypotheses, a wavefront per draw (three from an epoch's second round on), with PCL's stopping rule replayed in draw order; refinement
//                  (:117-126); the inlier bits (:128-133); the record
// A block of k_rp_estimate asks for 79 376 bytes of LDS, so that two blocks share a CU (160 KiB): one block's scattered
// gather hides under the other's hypothesis rounds.  What the block holds ("RANSAC planes for a batch"):
//   the sample as three float arrays                                  72 000 B
//   the RANSAC inliers as a bitmask over sample positions + prefix     1 136 B
//   the models, counts and list of valid draws of an epoch (256)       6 144 B
//   small counters                                                        96 B
// The original indices of a thread's (up to 12) sample points stay in its registers; the 256 partial sums of the
// refinement are assembled over the sample once every thread has taken what it needs from it.
//
// This translation unit uses the depth path through its public C-ABI only (mld_get_stream) and shares no internals with
// it (descriptor ring, object skeleton and compaction scratch: ../batch/mld_batch_object.h; the compaction's device
// pieces, load_xyz and the Jacobi: ../batch/mld_batch_device.h).  The results are nevertheless bit for bit those
// of mld_estimate_ground_plane (tests/test_ransac_planes_gpu.py pins that): the helpers - mix, sample_pos,
// plane_from, the distance, the stopping rule, the Jacobi - restate that path's arithmetic, and the float sums of
// the refinement keep its association: inlier q of the ordered list into partial q % 256, the partials in index order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../batch/mld_batch_object.h"
#include "../batch/mld_batch_device.h"

namespace {

using namespace mld_batch;

constexpr int kSample = 6000;   // RansacPlane.cpp:32
constexpr int kPartials = 256;

// the streaming kernel of the pass-through
constexpr int kPassBlock = 256;
constexpr int kGroupsPerWave = 4;
constexpr int kChunk = kPassBlock * kGroupsPerWave;  // 1024 points = 16 groups of 64 per block

// the estimator
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / kWave;                        // hypotheses evaluated per round
constexpr int kPerThread = (kSample + kThreads - 1) / kThreads;  // sample points per thread (12)
constexpr int kEpoch = 256;                                     // draws whose models are set up together
constexpr int kLater = 3;                                       // draws per wavefront and round after the first round (4 would
                                                                // need a 129th register: profiles/ransac_planes.md)
constexpr int kSampleWords = (kSample + kWave - 1) / kWave;     // 64-bit words of a bitmask over sample positions (94)
static_assert(kSampleWords <= 2 * kWave, "one wavefront scans the word counts, two per lane");
static_assert(kPartials * 9 <= 3 * kSample, "the partial sums fit over the dead sample");

// LDS of k_rp_estimate, in bytes from the start of the dynamic block
constexpr int kOffSample = 0;                                    // float sx[6000], sy[6000], sz[6000]
constexpr int kOffInl = kOffSample + 3 * kSample * 4;            // uint64 inl[94]
constexpr int kOffPre = kOffInl + kSampleWords * 8;              // int wpre[96]
constexpr int kOffModels = kOffPre + 96 * 4;                     // float mc[256][4]
constexpr int kOffCount = kOffModels + kEpoch * 16;              // int mcount[256]
constexpr int kOffList = kOffCount + kEpoch * 4;                 // int vlist[256]
constexpr int kOffMisc = kOffList + kEpoch * 4;                  // int wcnt[8], misc[16]
constexpr int kLdsBytes = kOffMisc + (kWaves + 16) * 4;
static_assert(kOffInl % 16 == 0 && kOffModels % 16 == 0, "16-byte LDS loads");
static_assert(kLdsBytes <= 80 * 1024, "two blocks per CU");

// One sequence of one call.  Host-made, staged through the descriptor ring (mld_batch::DescRing).
struct RpSeq {
    const unsigned char* cloud;
    uint32_t* mask;
    int32_t n;
    uint32_t seed;
};
static_assert(sizeof(RpSeq) == 24, "24 bytes per sequence (DESIGN.md)");
static_assert(sizeof(mld_ransac_plane_result) == 32, "mld.h");

// The estimator's parameters (mld_params.ransac_plane_*), by value to the kernels.
struct RpParams {
    double probability, thr, refine_thr;
    int32_t n_draws, max_it, use_refinement, pass;
    float lo, hi;
};

__host__ __device__ inline uint32_t mix(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t h = a * 0x9E3779B1u;
    h ^= b + 0x85EBCA6Bu + (h << 6) + (h >> 2);
    h ^= c * 0xC2B2AE35u + (h << 6) + (h >> 2);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// Stratified sub-sample (restatement of pcl::RandomSample, :66-74): position of sample point j among M candidates.
__device__ inline int sample_pos(int M, int j, uint32_t seed) {
    long long pos = j;
    if (M > kSample) {
        const double u = (double)mix(seed, (uint32_t)j, 0x5A17u) * (1.0 / 4294967296.0);
        pos = (long long)(((double)j + u) * (double)M / (double)kSample);
        if (pos > M - 1) pos = M - 1;
    }
    return (int)pos;
}

struct Model {
    float c[4];
    int degenerate;
    int valid;
};

// sac_model_plane computeModelCoefficients + sac_model_perpendicular_plane isModelValid, float arithmetic
__device__ inline Model plane_from(const float* p0, const float* p1, const float* p2) {
    Model m;
    float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
    float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
    float r0 = a0 / b0, r1 = a1 / b1, r2 = a2 / b2;
    m.degenerate = ((r0 == r1) && (r2 == r1)) ? 1 : 0;
    float n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
    float nn = sqrtf(n0 * n0 + n1 * n1 + n2 * n2);
    n0 /= nn;
    n1 /= nn;
    n2 /= nn;
    m.c[0] = n0;
    m.c[1] = n1;
    m.c[2] = n2;
    m.c[3] = -1.0f * (n0 * p0[0] + n1 * p0[1] + n2 * p0[2]);
    if (!(nn > 0.0f) || !isfinite(nn)) m.degenerate = 1;
    m.valid = (!m.degenerate && (fabs((double)n2) >= 0.984807753012208)) ? 1 : 0;  // cos(pi/18): 10 degrees
    return m;
}

// k-th (0-based) set bit of m; m has more than k set bits
__device__ inline int select_bit(unsigned long long m, int k) {
    int pos = 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << sh) - 1ull));
        if (k >= c) {
            k -= c;
            pos += sh;
        }
    }
    return pos;
}

// Inliers of NM planes among the S sample points (three coordinate arrays in LDS), by one wavefront: a lane reads four
// consecutive points with three 16-byte LDS loads - once for all NM planes.  Two points per instruction (the same IEEE
// operations as the scalar distance, no contraction), the inliers counted from the comparison masks.  out[m] is
// wavefront-uniform.
template <int NM>
__device__ inline void count_inliers(const float* sx, const float* sy, const float* sz, int S, int lane, float thr_f,
                                     const float (&c)[NM][4], int (&out)[NM]) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    int cnt[NM], cnt_wave[NM];  // per lane (the ragged end of the sample) / per wavefront
#pragma unroll
    for (int m = 0; m < NM; m++) cnt[m] = cnt_wave[m] = 0;
    auto four = [&](int j0) {  // four consecutive points per lane
        const f4 x = *reinterpret_cast<const f4*>(sx + j0), y = *reinterpret_cast<const f4*>(sy + j0),
                 z = *reinterpret_cast<const f4*>(sz + j0);
#pragma unroll
        for (int m = 0; m < NM; m++) {
            const f2 C0 = {c[m][0], c[m][0]}, C1 = {c[m][1], c[m][1]}, C2 = {c[m][2], c[m][2]}, C3 = {c[m][3], c[m][3]};
            const f2 da = ((C0 * x.xy + C1 * y.xy) + C2 * z.xy) + C3;
            const f2 db = ((C0 * x.zw + C1 * y.zw) + C2 * z.zw) + C3;
            cnt_wave[m] += __popcll(__ballot(fabsf(da.x) < thr_f)) + __popcll(__ballot(fabsf(da.y) < thr_f)) +
                           __popcll(__ballot(fabsf(db.x) < thr_f)) + __popcll(__ballot(fabsf(db.y) < thr_f));
        }
    };
    const int n_full = (S >> 2) / kWave;  // iterations in which every lane holds four points
    for (int it = 0; it < n_full; it++) four(4 * lane + it * (4 * kWave));
    const int j0 = 4 * lane + n_full * (4 * kWave);
    if (j0 + 3 < S) {
        // (not every lane is here: the ballots count the lanes that are)
        four(j0);
    } else {
        for (int j = j0; j < S; j++)  // the ragged end of the sample
#pragma unroll
            for (int m = 0; m < NM; m++)
                cnt[m] += (fabsf(c[m][0] * sx[j] + c[m][1] * sy[j] + c[m][2] * sz[j] + c[m][3]) < thr_f) ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < NM; m++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[m] += __shfl_xor(cnt[m], o);
        out[m] = cnt[m] + cnt_wave[m];
    }
}

// pcl::PassThrough on z with float limits (:57-64): candidate = finite && lo <= z <= hi.  Grid (sequence, chunk of 1024
// points).  gm: one 64-bit mask per 64 points, cpre[c + 1]: the candidates of chunk c (k_rp_scan makes them a prefix).
template <int kStride>
__global__ __launch_bounds__(kPassBlock) void k_rp_pass(const RpSeq* __restrict__ desc, float lo, float hi,
                                                       unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                       int* __restrict__ cpre_all, long long chunks_per_seq) {
    __shared__ int wsum[kPassBlock / kWave];
    const RpSeq q = desc[blockIdx.x];
    const int n = q.n;
    if ((int)blockIdx.y * kChunk >= n) return;  // (uniform in the block; max_points < 2^23: no overflow)
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x >> 6;
    const int first = ((int)blockIdx.y * (kPassBlock / kWave) + wave) * kGroupsPerWave * kWave;  // the wavefront's first point
    unsigned long long* __restrict__ gm = gm_all + (size_t)blockIdx.x * (size_t)groups_per_seq;
    float x[kGroupsPerWave], y[kGroupsPerWave], z[kGroupsPerWave];
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i = first + k * kWave + lane;
        x[k] = y[k] = z[k] = 0.f;
        if (i < n) load_xyz<kStride>(q.cloud, (uint32_t)i, x[k], y[k], z[k]);
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kGroupsPerWave; k++) {
        const int i0 = first + k * kWave;
        const bool f = (i0 + lane < n) && isfinite(x[k]) && isfinite(y[k]) && isfinite(z[k]) && !(z[k] < lo) && !(z[k] > hi);
        const unsigned long long m = __ballot(f);
        if (lane == 0 && i0 < n) *as_global(gm + (i0 >> 6)) = m;
        cnt += (int)__popcll(m);
    }
    if (lane == 0) wsum[wave] = cnt;
    chunk_count(wsum, cpre_all, chunks_per_seq);
}

// Exclusive prefix over the chunk counts of a sequence, in place: cpre[c] = candidates ahead of chunk c, cpre[NC] = all.
__global__ __launch_bounds__(256) void k_rp_scan(const RpSeq* __restrict__ desc, int* __restrict__ cpre_all,
                                                long long chunks_per_seq) {
    const int n = desc[blockIdx.x].n;
    const int NC = (n + kChunk - 1) / kChunk;
    (void)scan_chunk_counts(cpre_all + (size_t)blockIdx.x * (size_t)(chunks_per_seq + 1), NC);
}

// One block per sequence: the whole estimator.  Four wavefronts per SIMD (at most 128 registers): two blocks per CU.
template <int kStride>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_rp_estimate(const RpSeq* __restrict__ desc, RpParams P,
                                                         const unsigned long long* __restrict__ gm_all, long long groups_per_seq,
                                                         const int* __restrict__ cpre_all, long long chunks_per_seq,
                                                         mld_ransac_plane_result* __restrict__ res) {
    extern __shared__ __align__(16) unsigned char rp_smem[];
    float* sx = reinterpret_cast<float*>(rp_smem + kOffSample);
    float* sy = sx + kSample;
    float* sz = sy + kSample;
    unsigned long long* inl = reinterpret_cast<unsigned long long*>(rp_smem + kOffInl);  // RANSAC inliers by sample position
    int* wpre = reinterpret_cast<int*>(rp_smem + kOffPre);      // [g]: inliers in the words ahead of word g
    float* mc = reinterpret_cast<float*>(rp_smem + kOffModels);  // [kEpoch][4] model of the draw
    int* mcount = reinterpret_cast<int*>(rp_smem + kOffCount);  // [kEpoch] its inliers; 0: model not valid; -1: skipped draw
    int* vlist = reinterpret_cast<int*>(rp_smem + kOffList);    // [kEpoch] the epoch's valid draws, in order
    int* wcnt = reinterpret_cast<int*>(rp_smem + kOffMisc);     // [kWaves]
    int* misc = wcnt + kWaves;                                  // [0] inliers of the best model, [1] inlier total
    float* acc = sx;                                            // [kPartials * 9], once the sample is dead

    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    const int s = (int)blockIdx.x;
    const RpSeq q = desc[s];
    const int n = q.n;
    const uint32_t seed = q.seed;
    MLD_BATCH_GLOBAL uint32_t* gmask = as_global(q.mask);
    mld_ransac_plane_result* r = res + s;

    // the mask words are cleared before anything else: every way out below leaves a mask of zeros behind
    const int mask_words = (n + 31) >> 5;
    for (int i = tid; i < mask_words; i += kThreads) gmask[i] = 0u;

    const unsigned long long* __restrict__ gm = gm_all + (size_t)s * (size_t)groups_per_seq;
    const int* __restrict__ cpre = cpre_all + (size_t)s * (size_t)(chunks_per_seq + 1);
    const int G = (n + kWave - 1) / kWave, NC = (n + kChunk - 1) / kChunk;
    const int M = P.pass ? cpre[NC] : n;  // candidates
    const int S = M > kSample ? kSample : M;
    auto fail = [&]() {
        if (tid == 0) {
            r->coeffs[0] = r->coeffs[1] = r->coeffs[2] = r->coeffs[3] = 0.0f;
            r->n_inliers = 0;
            r->iterations = 0;
            r->status = 1;
            r->n_candidates = M;
        }
    };
    if (M < 3) {  // RansacPlane.cpp:44-50 (uniform in the block)
        fail();
        return;
    }
    // "(double)distance < thr" for a float distance == "distance < thr_f" with thr_f the smallest float >= thr
    auto up = [](double t) {
        float f = (float)t;
        if ((double)f < t) f = nextafterf(f, __builtin_huge_valf());
        return f;
    };
    const float thr_f = up(P.thr), sel_thr = up(P.use_refinement ? P.refine_thr : P.thr);
    const double log_probability = log(1.0 - P.probability);

    // ---- the sample: original indices of this thread's points j = tid, tid + 512, ... (they stay in registers for the
    // inlier bits), then all of the thread's cloud reads in flight at once ----
    uint32_t ids[kPerThread];
#pragma unroll
    for (int t = 0; t < kPerThread; t++) {
        const int j = tid + t * kThreads;
        ids[t] = 0u;
        if (j >= S) continue;
        const int pos = sample_pos(M, j, seed);
        if (!P.pass) {
            ids[t] = (uint32_t)pos;
            continue;
        }
        // the pos-th candidate: binary search over the chunk prefix, a walk over the (up to 16) group masks of that
        // chunk, a bit select
        int a = 0, b = NC;  // cpre[a] <= pos < cpre[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (cpre[mid] <= pos) a = mid; else b = mid;
        }
        int rest = pos - cpre[a], g = 16 * a;
        unsigned long long m = gm[g];
        while (g < G - 1 && rest >= (int)__popcll(m)) {
            rest -= (int)__popcll(m);
            m = gm[++g];
        }
        ids[t] = (uint32_t)(g * kWave + select_bit(m, rest));
    }
    {
        float px[kPerThread], py[kPerThread], pz[kPerThread];
#pragma unroll
        for (int t = 0; t < kPerThread; t++) {
            px[t] = py[t] = pz[t] = 0.0f;
            if (tid + t * kThreads < S) load_xyz<kStride>(q.cloud, ids[t], px[t], py[t], pz[t]);
        }
#pragma unroll
        for (int t = 0; t < kPerThread; t++) {
            const int j = tid + t * kThreads;
            if (j < S) {
                sx[j] = px[t];
                sy[j] = py[t];
                sz[j] = pz[t];
            }
        }
    }
    if (tid == 0) {
        misc[0] = 0;
        misc[1] = 0;
    }
    __syncthreads();

    // point j of the sample / its distance to a model
    auto dist = [&](const float c[4], int j) { return fabsf(c[0] * sx[j] + c[1] * sy[j] + c[2] * sz[j] + c[3]); };
    auto model_of = [&](int d) {  // the model of draw d
        uint32_t a = mix(seed, (uint32_t)d, 1u) % (uint32_t)S;
        uint32_t b = mix(seed, (uint32_t)d, 2u) % (uint32_t)S;
        uint32_t c = mix(seed, (uint32_t)d, 3u) % (uint32_t)S;
        if (b == a) b = (b + 1) % (uint32_t)S;
        while (c == a || c == b) c = (c + 1) % (uint32_t)S;
        const float p0[3] = {sx[a], sy[a], sz[a]}, p1[3] = {sx[b], sy[b], sz[b]}, p2[3] = {sx[c], sy[c], sz[c]};
        return plane_from(p0, p1, p2);
    };

    // ---- hypotheses.  The models of an epoch of draws are set up lane-parallel; only the draws whose model is valid
    // need their inliers counted, so a round hands the next VALID draws to the wavefronts.  PCL's sequential loop
    // (ransac.hpp computeModel: adaptive bound k = log(1-p)/log(1-w^3), skipped draws do not count as iterations, stop
    // at iterations >= k or > max_iterations) is replayed over the draws in order by every thread on the same data. ----
    int iterations = 0, best = -2147483647, best_draw = -1;
    double k = 1.0;
    const double one_over = 1.0 / (double)S;
    bool done = false;
    const int n_draws = P.n_draws, max_it = P.max_it;
    for (int e0 = 0, cap = 0; e0 < n_draws && !done; e0 += cap) {
        // the first epoch is one wavefront's worth of draws: most sequences stop within it
        cap = e0 == 0 ? kWave : kEpoch;
        const int ne = n_draws - e0 < cap ? n_draws - e0 : cap;
        const int dl = tid;  // this thread's draw of the epoch
        bool v = false;
        if (dl < ne) {
            const Model m = model_of(e0 + dl);
            v = m.valid != 0;
#pragma unroll
            for (int t = 0; t < 4; t++) mc[4 * dl + t] = m.c[t];
            mcount[dl] = m.degenerate ? -1 : 0;
        }
        const unsigned long long vm = __ballot(v);
        if (lane == 0) wcnt[w] = __popcll(vm);
        __syncthreads();
        int nv = 0, off = 0;
#pragma unroll
        for (int t = 0; t < kWaves; t++) {
            const int c = wcnt[t];
            off += t < w ? c : 0;
            nv += c;
        }
        if (v) vlist[off + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(vm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vm, 0u))] = dl;
        __syncthreads();
        int next = 0;  // draws of the epoch replayed so far
        for (int v0 = 0, round_n = 0; !done && next < ne; v0 += round_n) {
            // the first round decides most sequences with one draw per wavefront; one that goes on needs many more (a
            // small inlier share): kLater draws per wavefront from then on, the sample read once for all of them
            const int per = v0 == 0 ? 1 : kLater, first = v0 + w * per;
            round_n = kWaves * per;
            if (first < nv) {
                typedef float f4 __attribute__((ext_vector_type(4)));
                if (per == 1) {
                    const int d = vlist[first];
                    const f4 mq = *reinterpret_cast<const f4*>(mc + 4 * d);
                    const float c1[1][4] = {{mq.x, mq.y, mq.z, mq.w}};
                    int n1[1];
                    count_inliers<1>(sx, sy, sz, S, lane, thr_f, c1, n1);
                    if (lane == 0) mcount[d] = n1[0];
                } else {
                    const int mine = nv - first < kLater ? nv - first : kLater;
                    int ds[kLater], nl[kLater];
                    float cl[kLater][4];
#pragma unroll
                    for (int t = 0; t < kLater; t++) {  // (the last draw again where the list ends)
                        ds[t] = vlist[first + (t < mine ? t : mine - 1)];
                        const f4 mq = *reinterpret_cast<const f4*>(mc + 4 * ds[t]);
                        cl[t][0] = mq.x;
                        cl[t][1] = mq.y;
                        cl[t][2] = mq.z;
                        cl[t][3] = mq.w;
                    }
                    count_inliers<kLater>(sx, sy, sz, S, lane, thr_f, cl, nl);
#pragma unroll
                    for (int t = 0; t < kLater; t++)
                        if (lane == 0 && t < mine) mcount[ds[t]] = nl[t];
                }
            }
            __syncthreads();
            // every draw ahead of the next valid one that has not been counted yet can be replayed now
            const int upto = v0 + round_n < nv ? vlist[v0 + round_n] : ne;
            auto one_draw = [&](int c, int draw) {  // the reference's loop body; false: stop
                if (!((double)iterations < k)) return false;
                if (c < 0) return true;  // skipped draw
                if (c > best) {
                    best = c;
                    best_draw = draw;
                    const double wr = (double)best * one_over;
                    double p_no = 1.0 - wr * wr * wr;
                    p_no = fmax(2.220446049250313e-16, p_no);
                    p_no = fmin(1.0 - 2.220446049250313e-16, p_no);
                    k = log_probability / log(p_no);
                }
                ++iterations;
                return !(iterations > max_it);
            };
            // The counts of 64 draws are fetched at once; the runs of draws that neither improve on the best model nor
            // reach a stopping rule are booked in one step.
            while (next < upto && !done) {
                const int nb = upto - next < kWave ? upto - next : kWave;
                const int c = lane < nb ? mcount[next + lane] : -1;
                const unsigned long long counted = __ballot(c >= 0);
                int pos = 0;
                while (pos < nb && !done) {
                    const unsigned long long rest = ~0ull << pos;
                    const unsigned long long better = __ballot(c > best) & counted & rest;
                    const int ipos = better ? __ffsll((long long)better) - 1 : nb;  // the next draw that improves
                    const unsigned long long run = counted & rest & (ipos < kWave ? ~(~0ull << ipos) : ~0ull);
                    const int m = __popcll(run);  // counted draws ahead of it
                    // first iteration counts at which the rules stop the loop: !(i < k) before a draw, i > max_it after one
                    const int stop_k = k >= 2147483647.0 ? 2147483647 : (int)ceil(k);
                    if (iterations + m < stop_k && iterations + m <= max_it) {
                        iterations += m;  // none of them stops the loop
                        pos = ipos;
                        if (ipos < nb) {
                            if (!one_draw(__shfl(c, ipos), e0 + next + ipos)) done = true;
                            pos = ipos + 1;
                        }
                    } else {  // a stopping rule fires within the run (or right after it): draw by draw
                        const int end = ipos < nb ? ipos + 1 : nb;
                        for (; pos < end && !done; pos++)
                            if (!one_draw(__shfl(c, pos), e0 + next + pos)) done = true;
                    }
                }
                next += nb;
            }
        }
        __syncthreads();  // the next epoch rewrites the models and counts
    }
    if (best_draw < 0) {  // every draw was skipped: no model (uniform in the block)
        fail();
        return;
    }
    const Model bm = model_of(best_draw);
    const float rm[4] = {bm.c[0], bm.c[1], bm.c[2], bm.c[3]};
    float coeffs[4] = {rm[0], rm[1], rm[2], rm[3]};
    const bool valid = fabs((double)rm[2]) >= 0.984807753012208;

    // ---- the RANSAC inliers as a bitmask over sample positions (wavefront w takes the words w, w + 8, ...: position
    // 64 * word + lane is this thread's point tid + 512 t), and this thread's points of the FINAL set: the RANSAC inliers,
    // or (with refinement) the sample points within refinement_treshold of the UNREFINED model ----
    const int n_words = (S + kWave - 1) / kWave;
    unsigned fin_bits = 0u;
#pragma unroll
    for (int t = 0; t < kPerThread; t++) {
        const int j = tid + t * kThreads, g = w + t * kWaves;
        if (g >= n_words) break;  // (uniform in the wavefront)
        const float d = (j < S && valid) ? dist(rm, j) : __builtin_huge_valf();
        const unsigned long long m = __ballot(d < thr_f);
        if (lane == 0) inl[g] = m;
        fin_bits |= (d < sel_thr) ? (1u << t) : 0u;
    }
    __syncthreads();
    if (w == 0) {  // exclusive prefix of the words' counts, two words per lane
        const int v0 = lane < n_words ? (int)__popcll(inl[lane]) : 0;
        const int v1 = kWave + lane < n_words ? (int)__popcll(inl[kWave + lane]) : 0;
        int i0 = v0, i1 = v1;  // (not scan_inclusive: it costs this kernel three instructions, profiles/batch_device_header.md)
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int t0 = __shfl_up(i0, d), t1 = __shfl_up(i1, d);
            if (lane >= d) {
                i0 += t0;
                i1 += t1;
            }
        }
        const int total0 = __shfl(i0, kWave - 1);
        if (lane < n_words) wpre[lane] = i0 - v0;
        if (kWave + lane < n_words) wpre[kWave + lane] = total0 + i1 - v1;
        if (lane == kWave - 1) misc[0] = total0 + i1;
    }
    __syncthreads();
    const int ni = misc[0];
    if (P.use_refinement && ni > 3) {  // (uniform in the block)
        // optimizeModelCoefficients: thread p owns the inliers p, p + 256, ... of the ordered list - found by walking
        // the prefix forward - and the partials are combined in index order
        float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (tid < kPartials) {
            int g = 0;
            for (int o = tid; o < ni; o += kPartials) {
                while (g + 1 < n_words && wpre[g + 1] <= o) g++;
                const int jq = g * kWave + select_bit(inl[g], o - wpre[g]);
                const float v[3] = {sx[jq], sy[jq], sz[jq]};
                a[0] += v[0] * v[0];
                a[1] += v[0] * v[1];
                a[2] += v[0] * v[2];
                a[3] += v[1] * v[1];
                a[4] += v[1] * v[2];
                a[5] += v[2] * v[2];
                a[6] += v[0];
                a[7] += v[1];
                a[8] += v[2];
            }
        }
        __syncthreads();  // the sample is dead from here on: the partial sums take its place
        if (tid < kPartials)
            for (int t = 0; t < 9; t++) acc[tid * 9 + t] = a[t];
        __syncthreads();
        float mine = 0.0f;
        if (tid < 9) {
            float sum = 0.0f;
#pragma unroll 16
            for (int p = 0; p < kPartials; p++) sum += acc[p * 9 + tid];
            mine = sum / (float)ni;
        }
        __syncthreads();
        if (tid < 9) acc[tid] = mine;
        __syncthreads();
        if (tid == 0) {
            float s9[9];
            for (int t = 0; t < 9; t++) s9[t] = acc[t];
            float cov[6] = {s9[0] - s9[6] * s9[6], s9[1] - s9[6] * s9[7], s9[2] - s9[6] * s9[8],
                            s9[3] - s9[7] * s9[7], s9[4] - s9[7] * s9[8], s9[5] - s9[8] * s9[8]};
            double sd[6] = {cov[0], cov[1], cov[2], cov[3], cov[4], cov[5]}, n0[3];
            smallest_eigvec(sd, n0);
            const float e0 = (float)n0[0], e1 = (float)n0[1], e2 = (float)n0[2];
            coeffs[0] = e0;
            coeffs[1] = e1;
            coeffs[2] = e2;
            coeffs[3] = -1.0f * (e0 * s9[6] + e1 * s9[7] + e2 * s9[8]);
        }
    }
    // ---- the final inlier set, keyed by original index.  A stratified sample may name a point twice: the values the
    // atomics return tell, and such a point counts once.  (The words were cleared by this block, many barriers ago.) ----
    int cnt = 0;
    {
        uint32_t prev[kPerThread], bits[kPerThread];
#pragma unroll
        for (int t = 0; t < kPerThread; t++) {
            const bool in = (fin_bits >> t) & 1u;
            bits[t] = 1u << (ids[t] & 31);
            prev[t] = in ? atomicOr(q.mask + (ids[t] >> 5), bits[t]) : bits[t];
        }
#pragma unroll
        for (int t = 0; t < kPerThread; t++) cnt += (prev[t] & bits[t]) ? 0 : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) atomicAdd(&misc[1], cnt);
    __syncthreads();
    if (tid == 0) {
        for (int t = 0; t < 4; t++) r->coeffs[t] = coeffs[t];
        r->n_inliers = misc[1];
        r->iterations = iterations;
        r->status = 0;
        r->n_candidates = M;
    }
}

char g_error[512] = "";  // refusals without an object: mld_ransac_planes_last_error(NULL)

}  // namespace

struct mld_ransac_planes : mld_batch::Object {
    int n_seq = 0;
    int64_t max_points = 0;
    RpParams P{};
    CompactScratch scratch;  // pass-through: candidate mask per group; candidates ahead of every chunk (+ the total)
    mld_batch::DescRing<RpSeq> ring;
};

namespace {

int allocate(mld_ransac_planes* rp) {
    const int rc = rp->ring.allocate(rp, rp->n_seq);
    if (rc) return rc;
    const int rs = rp->scratch.allocate(rp, rp->n_seq, rp->max_points, kChunk, 1);
    if (rs) return rs;
    // (the limit on dynamic LDS is an attribute of the function on a device)
    MLD_HIP(rp, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rp_estimate<16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kLdsBytes));
    MLD_HIP(rp, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rp_estimate<32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kLdsBytes));
    return MLD_OK;
}

template <int kStride>
void launch_all(mld_ransac_planes* rp, int chunks, mld_ransac_plane_result* res) {
    const unsigned S = (unsigned)rp->n_seq;
    const CompactScratch& cs = rp->scratch;
    if (rp->P.pass) {
        if (chunks > 0)
            hipLaunchKernelGGL(k_rp_pass<kStride>, dim3(S, (unsigned)chunks), dim3(kPassBlock), 0, rp->stream, rp->ring.d_desc.get(),
                               rp->P.lo, rp->P.hi, cs.d_gm.get(), cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq);
        hipLaunchKernelGGL(k_rp_scan, dim3(S), dim3(256), 0, rp->stream, rp->ring.d_desc.get(), cs.d_cpre.get(), cs.chunks_per_seq);
    }
    hipLaunchKernelGGL(k_rp_estimate<kStride>, dim3(S), dim3(kThreads), kLdsBytes, rp->stream, rp->ring.d_desc.get(), rp->P, cs.d_gm.get(),
                       cs.groups_per_seq, cs.d_cpre.get(), cs.chunks_per_seq, res);
}

}  // namespace

extern "C" {

mld_ransac_planes* mld_ransac_planes_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_params* params,
                                            int* status_out) {
    auto refusal = [&]() -> const char* {
        // (the sizes first: they are refused without a look at the context)
        if (n_seq < 1 || n_seq > 65536) return "mld_ransac_planes_create: n_seq must be in 1 .. 65536";
        if (max_points < 1 || max_points > kMaxPoints) return "mld_ransac_planes_create: max_points must be in 1 .. 8388607";
        if (!ctx) return "mld_ransac_planes_create: null context";
        if (!params) return "mld_ransac_planes_create: null params";
        if (params->ransac_plane_max_iterations < 0 || params->ransac_plane_max_iterations == 2147483647)
            return "mld_ransac_planes_create: params->ransac_plane_max_iterations must be in 0 .. 2^31 - 2";
        return nullptr;
    };
    auto init = [&](mld_ransac_planes* rp) {
        rp->n_seq = n_seq;
        rp->max_points = max_points;
        RpParams& P = rp->P;
        P.probability = params->ransac_plane_probability;
        P.thr = params->ransac_plane_distance_treshold;
        P.refine_thr = params->ransac_plane_refinement_treshold;
        P.max_it = params->ransac_plane_max_iterations;
        P.n_draws = P.max_it + 1;
        P.use_refinement = params->ransac_plane_use_refinement ? 1 : 0;
        P.pass = params->ransac_plane_min_z > -1001. ? 1 : 0;  // RansacPlane.cpp:57
        P.lo = (float)params->ransac_plane_min_z;
        P.hi = (float)params->ransac_plane_max_z;
        return allocate(rp);
    };
    return mld_batch::create_object<mld_ransac_planes>(g_error, "mld_ransac_planes_create", refusal(), ctx, status_out, init);
}

void mld_ransac_planes_destroy(mld_ransac_planes* rp) { mld_batch::destroy_object(rp); }

const char* mld_ransac_planes_last_error(const mld_ransac_planes* rp) { return rp ? rp->err.c_str() : g_error; }

int mld_ransac_planes_estimate_device(mld_ransac_planes* rp, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                                      const uint32_t* seeds, mld_ransac_plane_result* result_out_dev,
                                      uint32_t* const* mask_out_dev) {
    if (!rp) return no_object(g_error, "mld_ransac_planes_estimate_device", "rp");
#define RP_REFUSE(text) return fail(rp, MLD_ERR_INVALID_ARG, "mld_ransac_planes_estimate_device: " text)
    if (!pts_dev) RP_REFUSE("null table pts_dev");
    if (!n) RP_REFUSE("null table n");
    if (!seeds) RP_REFUSE("null array seeds");
    if (!result_out_dev) RP_REFUSE("null array result_out_dev");
    if (!mask_out_dev) RP_REFUSE("null table mask_out_dev");
    if (stride_bytes != 16 && stride_bytes != 32) RP_REFUSE("stride_bytes must be 16 or 32");
    const int S = rp->n_seq;
    int64_t longest = 0;
    for (int s = 0; s < S; s++) {
        if (n[s] < 0) RP_REFUSE("negative n");
        if (n[s] > rp->max_points)
            return fail(rp, MLD_ERR_CAPACITY, "mld_ransac_planes_estimate_device: n exceeds the max_points of the object");
        if (n[s] > 0) {
            if (!pts_dev[s]) RP_REFUSE("null array pts_dev of a sequence with points");
            if (!mask_out_dev[s]) RP_REFUSE("null array mask_out_dev of a sequence with points");
            if (misaligned(pts_dev[s], 3u) || misaligned(mask_out_dev[s], 3u))
                RP_REFUSE("pts_dev and mask_out_dev must be 4-byte aligned");
        }
        if (n[s] > longest) longest = n[s];
    }
#undef RP_REFUSE
    for (int s = 0; s < S; s++) {
        RpSeq& q = rp->ring.stage[(size_t)s];
        q.cloud = static_cast<const unsigned char*>(pts_dev[s]);
        q.mask = mask_out_dev[s];
        q.n = (int32_t)n[s];
        q.seed = seeds[s];
    }
    MLD_HIP(rp, hipSetDevice(rp->device));
    const int rc = rp->ring.upload(rp);
    if (rc) return rc;
    const int chunks = (int)((longest + kChunk - 1) / kChunk);  // (<= 8192)
    with_stride(stride_bytes, [&](auto stride) { launch_all<decltype(stride)::value>(rp, chunks, result_out_dev); });
    MLD_HIP(rp, hipGetLastError());
    return MLD_OK;
}

}  // extern "C"
