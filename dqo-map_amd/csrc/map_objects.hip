// The object stage of a mapping frame on the device: the caller-owned object table, and for a frame with detections the reference's
// detections_filter, ObjectsInitialization / Object.__init__, Occlusions_Check, the live MatchObject (Only_IOU) and remove_outlier
// (SLAM/multiprocess/quadrics.py:336-386, 429-538, 926-968, 1013-1217, 2397-2425, driven as mapper.py:155-163) in ONE launch of ONE
// workgroup; Object_Optimize_only over the flagged rows (quadrics.py:2234-2298) and record_iou (mapper.py:1512-1531) as one launch each.
// include/dqo_raster.h (dqo_objmap_frame) states the contract, tests/object_oracle.py restates every statement in numpy.
//
// Arithmetic: double, from the float32 table (the reference is float64; a frame is a few thousand operations per object), one rounding
// per statement (-ffp-contract=off); the depth statistics alone are float32, in sample order, as the reference's tensor arithmetic.
//
// Shape of dqo_objmap_frame (1024 lanes, lane i owns row i; every barrier sits in block-uniform control flow, every loop is bounded by
// a capacity, and what ends a walk is published in LDS before anyone acts on it):
//   filter      lane per detection for the four own tests; the dedupe against the accepted ones walks the detections in order on wave 0,
//               all lanes testing their own detection, the verdict a ballot
//   depth       30 lanes per detection fetch, one lane sums in sample order
//   project     lane per row -> bbox and camera z in LDS
//   occlusion   rows in order; all lanes test their visible row against row i, the first hit in order is an atomic minimum in LDS
//   match       detections in order; all lanes test their visible row: first break entry (minimum), best IoU (maximum of the double's
//               bits, ties to the lower row), then lane 0 does the detection's bookkeeping
//   new         wave 0, rows handed out by a ballot's prefix count
//   outliers    lane per row projects (centre, clipped covariance -> LDS), lane j walks the rows i < j of its category
//   compaction  order-preserving block scan; rows move down one at a time, all lanes copying, in ascending order
#include "dqo_common.h"
#include "dqo_sample_hash.h"
#include "dqo_quadric_eval.h"

namespace {

constexpr int OBJ_BLOCK = 1024;  // = the largest cap_obj
constexpr int OBJ_MAX_DET = 64;
constexpr int N_SAMPLES = 30;
constexpr int N_OPT_ITERS = 20;
enum { FATE_DROPPED = 0, FATE_INVALID, FATE_MATCHED, FATE_NEW, FATE_REPLACED, FATE_UNMATCHED };
enum { H_ACCEPTED = 0, H_MATCHED, H_NEW, H_REPLACED, H_REMOVED, H_HAS_NEW, H_OVER_OBJ, H_OVER_VIEWS };

struct ObjTable {
    int cap_obj, cap_views;
    float *axes, *R, *center;
    int32_t *cat, *uid, *nviews;
    float *view_P34, *view_bbox;
    int32_t* state;
};

struct ObjFrame {
    int M, W, H, frame_id;
    uint64_t seed;
    const float *bbox, *ellipse, *score, *depth, *K, *Rt;
    const int32_t* cat;
    int32_t *fate, *row;
    float* det_depth;
    uint8_t* opt_flag;
    int32_t* header;
};

__device__ __forceinline__ double area4(const double* b) { return (b[2] - b[0]) * (b[3] - b[1]); }

__device__ __forceinline__ double inter4(const double* a, const double* b) {
    const double w = fmax(fmin(a[2], b[2]) - fmax(a[0], b[0]), 0.0), h = fmax(fmin(a[3], b[3]) - fmax(a[1], b[1]), 0.0);
    return h * w;
}

__device__ __forceinline__ double iou4(const double* a, const double* b) {
    const double in = inter4(a, b);
    return in / (area4(a) + area4(b) - in);
}

// is_cover(bb1, bb2), quadrics.py:296-310
__device__ __forceinline__ bool is_cover(const double* a, const double* b) {
    const double in = inter4(a, b), aa = area4(a);
    if (aa == 0.0) return false;
    return in / aa > 0.5 && in / area4(b) < 0.5;
}

struct Proj {
    double mu[2], bbox[4], cov[3], ax_lo, ax_hi;  // cov: xx, xy, yy, clipped at 0 (AsGaussian)
};

// Ellipsoid.project + Ellipse.FromDual + decompose + ComputeBbox + AsGaussian (quadrics.py:148-248, 388-408), the 2x2 eigen-decomposition
// in closed form as in dqo_quadric_eval.h: ComputeBbox needs only the squared cosine and sine.
__device__ void project_row(const float* axes, const float* Rm, const float* ctr, const double* P, Proj& o) {
    double A[3], c[3], Q[4][4];
    for (int i = 0; i < 3; i++) A[i] = (double)axes[i] * (double)axes[i], c[i] = ctr[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)Rm[3 * i + k] * A[k] * (double)Rm[3 * j + k];
            Q[i][j] = s - c[i] * c[j];
        }
    for (int i = 0; i < 3; i++) Q[i][3] = Q[3][i] = -c[i];
    Q[3][3] = -1.0;
    double PQ[3][4], C[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += P[4 * i + k] * Q[k][j];
            PQ[i][j] = s;
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += PQ[i][k] * P[4 * j + k];
            C[i][j] = s;
        }
    const double nrm = -C[2][2];
    const double c00 = C[0][0] / nrm, c01 = 0.5 * (C[0][1] + C[1][0]) / nrm, c11 = C[1][1] / nrm;
    const double mux = -(0.5 * (C[0][2] + C[2][0]) / nrm), muy = -(0.5 * (C[1][2] + C[2][1]) / nrm);
    const double p = c00 + mux * mux, q = c01 + mux * muy, r = c11 + muy * muy;
    const double m = 0.5 * (p + r), hd = 0.5 * (p - r);
    const double h = sqrt(hd * hd + q * q);
    const double a_hi = fabs(m + h), a_lo = fabs(m - h);
    const double k = h > 0.0 ? hd / h : 0.0, kq = h > 0.0 ? q / h : 0.0;
    const double X = sqrt(a_lo * (0.5 * (1.0 - k)) + a_hi * (0.5 * (1.0 + k)));
    const double Y = sqrt(a_lo * (0.5 * (1.0 + k)) + a_hi * (0.5 * (1.0 - k)));
    o.mu[0] = mux, o.mu[1] = muy;
    o.bbox[0] = mux - X, o.bbox[1] = muy - Y, o.bbox[2] = mux + X, o.bbox[3] = muy + Y;
    const double hs = 0.5 * (a_hi + a_lo), hdif = 0.5 * (a_hi - a_lo);
    o.cov[0] = fmax(hs + hdif * k, 0.0), o.cov[1] = fmax(hdif * kq, 0.0), o.cov[2] = fmax(hs - hdif * k, 0.0);
    o.ax_lo = sqrt(a_lo), o.ax_hi = sqrt(a_hi);
}

// Calculate_distance(e1, e2, 10), quadrics.py:970-988, with its element-wise square roots.  e: mu x, mu y, cov xx, xy, yy
__device__ double wasserstein_score(const double* e1, const double* e2) {
    const double s0 = sqrt(e1[2]), s1 = sqrt(e1[3]), s2 = sqrt(e1[4]);  // sigma11 = [[s0, s1], [s1, s2]]
    // t = sigma11 @ sigma2
    const double t00 = s0 * e2[2] + s1 * e2[3], t01 = s0 * e2[3] + s1 * e2[4];
    const double t10 = s1 * e2[2] + s2 * e2[3], t11 = s1 * e2[3] + s2 * e2[4];
    // the diagonal of t @ sigma11
    const double u00 = t00 * s0 + t01 * s1, u11 = t10 * s1 + t11 * s2;
    const double dx = e1[0] - e2[0], dy = e1[1] - e2[1];
    double d = (dx * dx + dy * dy) + ((e1[2] + e2[2] - 2.0 * sqrt(u00)) + (e1[4] + e2[4] - 2.0 * sqrt(u11)));
    if (d < 0.0) d = 0.0;
    return exp(-sqrt(d) / 10.0);
}

// Object.__init__ (quadrics.py:451-482) into row `row`, with its first observation.  bb, P: the float32 values as stored
__device__ void write_object(const ObjTable& t, int row, int cat, int uid, const float* bb, const float* dd, const double* K, const double* Rt,
                             const float* Pst) {
    const double avg = dd[0], dif = dd[1];
    const double b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
    const double u = ((b0 + b2) / 2.0 - K[2]) / K[0], v = ((b1 + b3) / 2.0 - K[5]) / K[4];
    const double cam[3] = {u * avg, v * avg, avg};
    double ctr[3];
    for (int i = 0; i < 3; i++) {  // Rcw^T cam + (-Rcw^T tcw)
        const double a = (Rt[0 + i] * cam[0] + Rt[4 + i] * cam[1]) + Rt[8 + i] * cam[2];
        const double b = (-Rt[0 + i] * Rt[3] + -Rt[4 + i] * Rt[7]) + -Rt[8 + i] * Rt[11];
        ctr[i] = a + b;
    }
    const double n = sqrt((cam[0] * cam[0] + cam[1] * cam[1]) + cam[2] * cam[2]);
    const double zc[3] = {cam[0] / n, cam[1] / n, cam[2] / n};
    double xc[3] = {zc[2], 0.0, -zc[0]};  // cross((0, 1, 0), zc)
    const double nx = sqrt((xc[0] * xc[0] + xc[1] * xc[1]) + xc[2] * xc[2]);
    for (int i = 0; i < 3; i++) xc[i] = xc[i] / nx;
    const double yc[3] = {zc[1] * xc[2] - zc[2] * xc[1], zc[2] * xc[0] - zc[0] * xc[2], zc[0] * xc[1] - zc[1] * xc[0]};
    const double* col[3] = {xc, yc, zc};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)  // rot_world = Rcw^T rot_cam
            t.R[9 * row + 3 * i + j] = (float)((Rt[0 + i] * col[j][0] + Rt[4 + i] * col[j][1]) + Rt[8 + i] * col[j][2]);
    t.axes[3 * row + 0] = (float)((b2 - b0) * avg / K[0] * 0.5);
    t.axes[3 * row + 1] = (float)((b3 - b1) * avg / K[4] * 0.5);
    t.axes[3 * row + 2] = (float)(dif * 0.5);
    for (int i = 0; i < 3; i++) t.center[3 * row + i] = (float)ctr[i];
    t.cat[row] = cat, t.uid[row] = uid, t.nviews[row] = 1;
    const size_t slot = (size_t)row * t.cap_views;
    for (int i = 0; i < 12; i++) t.view_P34[slot * 12 + i] = Pst[i];
    for (int i = 0; i < 4; i++) t.view_bbox[slot * 4 + i] = bb[i];
}

__device__ __forceinline__ int trunc_clamped(float x) { return (int)fminf(fmaxf(x, -1.0e9f), 1.0e9f); }

__global__ void __launch_bounds__(OBJ_BLOCK) objmap_frame_kernel(ObjTable t, ObjFrame f) {
    // phase-shared storage: depth samples (filter), then bbox [4] + z per row (occlusion, match), then mu [2] + cov [3] per row (outliers)
    __shared__ double s_row[OBJ_BLOCK * 5];
    __shared__ double s_citou[OBJ_BLOCK];      // contest: the holder's IoU
    __shared__ int8_t s_cdet[OBJ_BLOCK];       // contest: the holder's detection, -1 none
    __shared__ uint8_t s_vis[OBJ_BLOCK], s_cand[OBJ_BLOCK], s_gone[OBJ_BLOCK];
    __shared__ int s_newidx[OBJ_BLOCK];
    __shared__ double s_dbox[OBJ_MAX_DET * 4];
    __shared__ float s_dd[OBJ_MAX_DET * 2];
    __shared__ float s_dbf[OBJ_MAX_DET * 4];
    __shared__ int s_dcat[OBJ_MAX_DET], s_fate[OBJ_MAX_DET], s_drow[OBJ_MAX_DET];
    __shared__ uint8_t s_acc[OBJ_MAX_DET], s_dobj[OBJ_MAX_DET], s_valid[OBJ_MAX_DET];
    __shared__ double s_K[9], s_Rt[12], s_P[12];
    __shared__ float s_Pst[12];
    __shared__ int s_hdr[8];
    __shared__ int s_first, s_best_idx, s_n, s_uid, s_wave_tot[OBJ_BLOCK / 64];
    __shared__ unsigned long long s_best_bits;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = f.M, W = f.W, H = f.H;
    const int cap_obj = t.cap_obj, cap_views = t.cap_views;
    const int n0 = min(max(t.state[0], 0), cap_obj);
    const int started = t.state[2];
    float* s_samp = reinterpret_cast<float*>(s_row);  // [OBJ_MAX_DET][32]

    if (tid < 9) s_K[tid] = f.K[tid];
    if (tid < 12) s_Rt[tid] = f.Rt[tid];
    if (tid < 8) s_hdr[tid] = 0;
    if (tid == 0) s_n = n0, s_uid = t.state[1], s_first = INT_MAX, s_best_idx = INT_MAX, s_best_bits = 0ull;
    for (int i = tid; i < cap_obj; i += OBJ_BLOCK) f.opt_flag[i] = 0;
    s_vis[tid] = 0, s_cand[tid] = 0, s_gone[tid] = 0, s_cdet[tid] = -1, s_citou[tid] = 0.0, s_newidx[tid] = tid;
    __syncthreads();
    if (tid < 12) {  // P = K @ Rt, and as the table stores it
        const int i = tid >> 2, j = tid & 3;
        const double p = (s_K[3 * i] * s_Rt[j] + s_K[3 * i + 1] * s_Rt[4 + j]) + s_K[3 * i + 2] * s_Rt[8 + j];
        s_P[tid] = p, s_Pst[tid] = (float)p;
    }

    // ---- detections_filter, quadrics.py:336-353: the four tests of a detection on its own ----
    bool own = false;
    if (tid < M) {
        double b[4], e[4];
        for (int i = 0; i < 4; i++) s_dbf[4 * tid + i] = f.bbox[4 * tid + i], b[i] = s_dbox[4 * tid + i] = f.bbox[4 * tid + i];
        s_dcat[tid] = f.cat[tid];
        const double area = area4(b), sc = f.score[tid];
        const float* el = f.ellipse + 5 * tid;  // centre, full axes, angle (the json's order, :262)
        const double a0 = 0.5 * (double)el[2], a1 = 0.5 * (double)el[3], cs = cos((double)el[4]), sn = sin((double)el[4]);
        const double X = sqrt((a0 * a0) * (cs * cs) + (a1 * a1) * (sn * sn)), Y = sqrt((a0 * a0) * (sn * sn) + (a1 * a1) * (cs * cs));
        e[0] = (double)el[0] - X, e[1] = (double)el[1] - Y, e[2] = (double)el[0] + X, e[3] = (double)el[1] + Y;
        own = !(sc < 0.2 || area < 300.0 || area > 0.5 * H * W || iou4(b, e) < 0.2);
        s_fate[tid] = FATE_DROPPED, s_drow[tid] = -1, s_dobj[tid] = 0, s_valid[tid] = 1, s_dd[2 * tid] = s_dd[2 * tid + 1] = 0.f;
    }
    __syncthreads();
    if (wave == 0) {  // the dedupe against the already accepted detections, in order (no barrier inside: one wave)
        bool acc = false;
        for (int d = 0; d < OBJ_MAX_DET; d++) {
            if (d >= M) break;  // (M is uniform)
            bool hit = false;
            if (lane < d && acc) {
                const double iou = iou4(&s_dbox[4 * d], &s_dbox[4 * lane]);
                hit = s_dcat[d] == s_dcat[lane] ? iou > 0.3 : iou > 0.6;
            }
            const bool any = __ballot(hit) != 0ull;
            if (lane == d) acc = own && !any;
        }
        if (lane < M) s_acc[lane] = acc ? 1 : 0;
        const unsigned long long am = __ballot(lane < M && acc);
        if (lane == 0) s_hdr[H_ACCEPTED] = __popcll(am);
    }
    __syncthreads();

    // ---- the depth statistics, :356-380: 30 samples by the key rule, summed in sample order in float32 ----
    for (int k = tid; k < OBJ_MAX_DET * 32; k += OBJ_BLOCK) {  // (two rounds: 64 detections of 32 slots over 1024 lanes)
        const int d = k >> 5, s = k & 31;
        if (d < M && s < N_SAMPLES && s_acc[d]) {
            const uint32_t sw = dqo_sample_seed_word(f.seed);
            const float* b = &s_dbf[4 * d];
            const int lo_u = trunc_clamped(b[0]), hi_u = trunc_clamped(b[2]), lo_v = trunc_clamped(b[1]), hi_v = trunc_clamped(b[3]);
            const uint32_t span_u = hi_u >= lo_u ? (uint32_t)((int64_t)hi_u - lo_u + 1) : 1u;
            const uint32_t span_v = hi_v >= lo_v ? (uint32_t)((int64_t)hi_v - lo_v + 1) : 1u;
            const int64_t uu = (int64_t)lo_u + dqo_object_key(sw, 8u, (uint32_t)f.frame_id, (uint32_t)(d * 32 + s)) % span_u;
            const int64_t vv = (int64_t)lo_v + dqo_object_key(sw, 9u, (uint32_t)f.frame_id, (uint32_t)(d * 32 + s)) % span_v;
            const int u = (int)min(max(uu, (int64_t)0), (int64_t)(W - 1)), v = (int)min(max(vv, (int64_t)0), (int64_t)(H - 1));
            s_samp[32 * d + s] = f.depth[(size_t)v * W + u];
        }
    }
    __syncthreads();
    if (tid < M && s_acc[tid]) {
        float sum_d = 0.f, min_d = 100.f, max_d = -1.f;
        int count = 0;
        for (int s = 0; s < N_SAMPLES; s++) {
            const float x = s_samp[32 * tid + s];
            if (x > 0.0f) {
                sum_d = sum_d + x;
                count++;
                if (x < min_d) min_d = x;
                if (x > max_d) max_d = x;
            }
        }
        if (count > 0) {
            const float avg = (float)((double)sum_d / (double)count);  // = the float32 quotient (a double quotient of floats rounds once)
            s_dd[2 * tid] = (float)fmin((double)avg, 5.0);
            s_dd[2 * tid + 1] = (float)fmin(fmax((double)(max_d - min_d), 0.05), 0.2);
        }
    }
    __syncthreads();  // (s_samp is dead from here: s_row is the rows')

    if (!started) {
        // ---- ObjectsInitialization, :514-538 (Map_global is None) ----
        if (wave == 0) {
            const bool accd = lane < M && s_acc[lane];
            const double avg = s_dd[2 * (lane < M ? lane : 0)];
            const bool good = accd && avg > 0.0 && avg < 15.0;
            const unsigned long long gm = __ballot(good);
            const int rank = __popcll(gm & ((1ull << lane) - 1ull)), total = __popcll(gm);
            if (accd) {
                int row = -1;
                if (good && n0 + rank < cap_obj) {
                    row = n0 + rank;
                    write_object(t, row, s_dcat[lane], s_uid + rank, &s_dbf[4 * lane], &s_dd[2 * lane], s_K, s_Rt, s_Pst);
                }
                s_fate[lane] = good ? FATE_NEW : FATE_UNMATCHED, s_drow[lane] = row;
            }
            if (lane == 0) {
                const int stored = min(total, cap_obj - n0);
                s_hdr[H_OVER_OBJ] = total - stored, s_hdr[H_HAS_NEW] = 1;
                s_n = n0 + stored, s_uid = s_uid + stored;
            }
        }
        __syncthreads();
    } else {
        // ---- Occlusions_Check, :926-968 ----
        double* s_bbox = s_row;                  // [OBJ_BLOCK][4]
        double* s_z = s_row + 4 * OBJ_BLOCK;     // [OBJ_BLOCK]
        double mybox[4] = {0, 0, 0, 0};
        if (tid < n0) {
            Proj pr;
            project_row(t.axes + 3 * tid, t.R + 9 * tid, t.center + 3 * tid, s_P, pr);
            const double z = ((s_Rt[8] * (double)t.center[3 * tid] + s_Rt[9] * (double)t.center[3 * tid + 1]) +
                              s_Rt[10] * (double)t.center[3 * tid + 2]) + s_Rt[11];
            for (int i = 0; i < 4; i++) s_bbox[4 * tid + i] = mybox[i] = pr.bbox[i];
            s_z[tid] = z;
            const double img[4] = {0.0, 0.0, (double)W, (double)H};
            s_cand[tid] = !(z < 0.0 || inter4(pr.bbox, img) < 0.3 * area4(pr.bbox)) ? 1 : 0;
        }
        __syncthreads();
        for (int i = 0; i < OBJ_BLOCK; i++) {
            if (i >= n0) break;  // (n0 is uniform)
            const bool cand = s_cand[i] != 0;  // uniform
            if (cand && tid < i && s_vis[tid] && iou4(mybox, &s_bbox[4 * i]) > 0.8) atomicMin(&s_first, tid);
            __syncthreads();
            if (tid == 0) {
                if (cand) {
                    const int j = s_first;
                    if (j == INT_MAX)
                        s_vis[i] = 1;
                    else if (s_z[i] < s_z[j])
                        s_vis[j] = 0, s_vis[i] = 1;  // the earlier entry is the farther one
                    s_first = INT_MAX;
                }
            }
            __syncthreads();
        }

        // ---- MatchObject, :1031-1160 ----
        const int mycat = tid < n0 ? t.cat[tid] : -1;  // (a covering replacement keeps the category: it needs an equal one)
        for (int d = 0; d < OBJ_MAX_DET; d++) {
            if (d >= M) break;
            const bool accd = s_acc[d] != 0;  // uniform
            const double* bd = &s_dbox[4 * d];
            const bool vis = accd && tid < n0 && s_vis[tid];
            double iou = 0.0;
            if (vis) {
                iou = iou4(mybox, bd);
                if (mycat == s_dcat[d] && iou < 0.5 && (is_cover(mybox, bd) || is_cover(bd, mybox))) atomicMin(&s_first, tid);
            }
            __syncthreads();
            const int brk = s_first;  // the entry the walk breaks at (INT_MAX: none)
            const bool runs = vis && tid < brk && iou > 0.5;
            if (runs) atomicMax(&s_best_bits, (unsigned long long)__double_as_longlong(iou));
            __syncthreads();
            if (runs && (unsigned long long)__double_as_longlong(iou) == s_best_bits) atomicMin(&s_best_idx, tid);
            __syncthreads();
            if (tid == 0 && accd) {
                double iou_max = 0.0;
                int node = -1;
                bool replaced = false;
                if (brk != INT_MAX) {
                    if (is_cover(&s_bbox[4 * brk], bd)) {  // the detection covers the stored object: a fresh Object takes its row
                        write_object(t, brk, s_dcat[d], s_uid, &s_dbf[4 * d], &s_dd[2 * d], s_K, s_Rt, s_Pst);
                        s_uid = s_uid + 1;
                        node = brk, iou_max = 1.0, replaced = true;
                    } else {
                        s_valid[d] = 0;
                    }
                } else if (s_best_idx != INT_MAX) {
                    node = s_best_idx, iou_max = __longlong_as_double((long long)s_best_bits);
                }
                bool keep = iou_max > 0.5;
                if (keep && !replaced) {  // last_obs_ids_and_max_iou, :1132-1151 (a fresh Object holds none)
                    const int holder = s_cdet[node];
                    if (holder >= 0) {
                        if (iou_max < s_citou[node])
                            keep = false;
                        else
                            s_dobj[holder] = 0;
                    }
                    if (keep) s_cdet[node] = (int8_t)d, s_citou[node] = iou_max;
                }
                if (keep) {
                    s_dobj[d] = 1, s_drow[d] = node, s_fate[d] = replaced ? FATE_REPLACED : FATE_MATCHED;
                    if (replaced) s_hdr[H_REPLACED] = s_hdr[H_REPLACED] + 1;
                    Proj pr;
                    project_row(t.axes + 3 * node, t.R + 9 * node, t.center + 3 * node, s_P, pr);
                    const bool skip = (iou4(pr.bbox, bd) < 0.01 && !s_valid[d]) || pr.ax_lo <= 0.001 || pr.ax_hi <= 0.001;
                    if (!skip) {
                        const int nv = t.nviews[node];
                        if (nv >= cap_views) {
                            s_hdr[H_OVER_VIEWS] = s_hdr[H_OVER_VIEWS] + 1;
                        } else {
                            const size_t slot = (size_t)node * cap_views + nv;
                            for (int i = 0; i < 12; i++) t.view_P34[slot * 12 + i] = s_Pst[i];
                            for (int i = 0; i < 4; i++) t.view_bbox[slot * 4 + i] = s_dbf[4 * d + i];
                            t.nviews[node] = nv + 1;
                        }
                    }
                }
            }
            if (tid == 0) s_first = INT_MAX, s_best_idx = INT_MAX, s_best_bits = 0ull;
            __syncthreads();
        }

        // ---- new objects, :1164-1186 ----
        if (wave == 0) {
            const bool accd = lane < M && s_acc[lane];
            const bool open = accd && !s_dobj[lane];
            const double avg = s_dd[2 * (lane < M ? lane : 0)];
            const bool good = open && s_valid[lane] && avg > 0.01 && avg < 15.0;
            const unsigned long long gm = __ballot(good);
            const int rank = __popcll(gm & ((1ull << lane) - 1ull)), total = __popcll(gm);
            if (open) {
                int row = -1;
                if (good && n0 + rank < cap_obj) {
                    row = n0 + rank;
                    write_object(t, row, s_dcat[lane], s_uid + rank, &s_dbf[4 * lane], &s_dd[2 * lane], s_K, s_Rt, s_Pst);
                }
                s_fate[lane] = !s_valid[lane] ? FATE_INVALID : (good ? FATE_NEW : FATE_UNMATCHED), s_drow[lane] = row;
            }
            if (lane == 0) {
                const int stored = min(total, cap_obj - n0);
                s_hdr[H_OVER_OBJ] = total - stored, s_hdr[H_HAS_NEW] = total > 0 ? 1 : 0;
                s_n = n0 + stored, s_uid = s_uid + stored;
            }
        }
        __syncthreads();

        // ---- remove_outlier, :2397-2425: row j goes when any row i < j of its category is far from it ----
        const int n1 = s_n;
        double* s_e = s_row;  // [OBJ_BLOCK][5]: mu, cov (the boxes are dead)
        double mine[5] = {0, 0, 0, 0, 0};
        int cat_j = -1;
        if (tid < n1) {
            Proj pr;
            project_row(t.axes + 3 * tid, t.R + 9 * tid, t.center + 3 * tid, s_P, pr);
            mine[0] = pr.mu[0], mine[1] = pr.mu[1], mine[2] = pr.cov[0], mine[3] = pr.cov[1], mine[4] = pr.cov[2];
            cat_j = t.cat[tid];
        }
        __syncthreads();  // (every lane has read its box of s_row)
        if (tid < n1)
            for (int i = 0; i < 5; i++) s_e[5 * tid + i] = mine[i];
        __syncthreads();
        bool gone = false;
        if (tid < n1)
            for (int i = 0; i < OBJ_BLOCK; i++) {
                if (i >= tid) break;
                if (t.cat[i] == cat_j && wasserstein_score(&s_e[5 * i], mine) < 0.1) gone = true;
            }
        // ---- compaction: an order-preserving scan of the kept rows, then the rows move down in ascending order ----
        const bool kept = tid < n1 && !gone;
        const unsigned long long km = __ballot(kept);
        if (lane == 0) s_wave_tot[wave] = __popcll(km);
        s_gone[tid] = (tid < n1 && gone) ? 1 : 0;
        __syncthreads();
        int base = 0, n2 = 0;
        for (int w = 0; w < OBJ_BLOCK / 64; w++) {
            if (w < wave) base += s_wave_tot[w];
            n2 += s_wave_tot[w];
        }
        s_newidx[tid] = base + __popcll(km & ((1ull << lane) - 1ull));
        __syncthreads();
        if (n2 != n1) {  // uniform
            for (int j = 0; j < OBJ_BLOCK; j++) {
                if (j >= n1) break;
                const int dst = s_newidx[j];
                if (!s_gone[j] && dst != j) {  // uniform
                    const int nv = min(max(t.nviews[j], 0), cap_views);
                    if (tid < 3) t.axes[3 * dst + tid] = t.axes[3 * j + tid], t.center[3 * dst + tid] = t.center[3 * j + tid];
                    if (tid < 9) t.R[9 * dst + tid] = t.R[9 * j + tid];
                    if (tid == 0) t.cat[dst] = t.cat[j], t.uid[dst] = t.uid[j];
                    for (int e = tid; e < nv * 12; e += OBJ_BLOCK)
                        t.view_P34[(size_t)dst * cap_views * 12 + e] = t.view_P34[(size_t)j * cap_views * 12 + e];
                    for (int e = tid; e < nv * 4; e += OBJ_BLOCK)
                        t.view_bbox[(size_t)dst * cap_views * 4 + e] = t.view_bbox[(size_t)j * cap_views * 4 + e];
                    __syncthreads();  // (nviews[j] is read by every lane before it moves)
                    if (tid == 0) t.nviews[dst] = nv;
                    __syncthreads();
                }
            }
            if (tid < M && s_drow[tid] >= 0) s_drow[tid] = s_gone[s_drow[tid]] ? -1 : s_newidx[s_drow[tid]];
            if (tid == 0) s_hdr[H_REMOVED] = n1 - n2, s_n = n2;
        }
        __syncthreads();
    }

    // ---- outputs; the gate of Object_Optimize_only, :2246-2249 ----
    if (tid < M) {
        const int fate = s_fate[tid], row = s_drow[tid];
        f.fate[tid] = fate, f.row[tid] = row;
        f.det_depth[2 * tid] = s_dd[2 * tid], f.det_depth[2 * tid + 1] = s_dd[2 * tid + 1];
        if ((fate == FATE_MATCHED || fate == FATE_NEW || fate == FATE_REPLACED) && row >= 0 && t.nviews[row] >= 2) f.opt_flag[row] = 1;
    }
    if (wave == 0) {
        const int fate = lane < M ? s_fate[lane] : -1;
        const int nm = __popcll(__ballot(fate == FATE_MATCHED)), nn = __popcll(__ballot(fate == FATE_NEW));
        if (lane < 8) {
            int v = s_hdr[lane];
            if (lane == H_MATCHED) v = nm;
            if (lane == H_NEW) v = nn;
            f.header[lane] = v;
        }
        if (lane == 0) t.state[0] = s_n, t.state[1] = s_uid, t.state[2] = 1;
    }
}

// Object_Optimize_only (quadrics.py:2234-2298) for every flagged row, reading the row's observation slots in place
__global__ void __launch_bounds__(64) objmap_optimize_kernel(ObjTable t, const uint8_t* __restrict__ opt_flag, int frame_id, uint64_t seed, float* __restrict__ loss_hist) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = min(max(t.state[0], 0), t.cap_obj);
    if (row >= n || !opt_flag[row]) return;
    const int nv = min(t.nviews[row], t.cap_views);
    if (nv < 1) return;
    float prm[15];
    for (int i = 0; i < 3; i++) prm[i] = t.axes[3 * row + i], prm[3 + i] = t.center[3 * row + i];
    for (int i = 0; i < 9; i++) prm[6 + i] = t.R[9 * row + i];
    const uint32_t sw = dqo_sample_seed_word(seed), uid = (uint32_t)t.uid[row];
    quadric_adam_lane(prm, N_OPT_ITERS, t.view_P34 + (size_t)row * t.cap_views * 12, t.view_bbox + (size_t)row * t.cap_views * 4,
                      [=](int it) {  // random.randint(0, len - 1) for it <= 5, the last observation afterwards (:2264-2266)
                          return it <= N_OPT_ITERS / 4 ? (int)(dqo_object_key(sw, 10u, (uint32_t)frame_id, uid * 32u + (uint32_t)it) % (uint32_t)nv)
                                                       : nv - 1;
                      },
                      loss_hist ? loss_hist + (size_t)row * N_OPT_ITERS : nullptr);
    for (int i = 0; i < 3; i++) t.axes[3 * row + i] = prm[i], t.center[3 * row + i] = prm[3 + i];
    for (int i = 0; i < 9; i++) t.R[9 * row + i] = prm[6 + i];
}

// record_iou (mapper.py:1512-1531): a row's mean IoU over its stored observations with IoU > 0, or 0 with none
__global__ void __launch_bounds__(64) objmap_mean_iou_kernel(ObjTable t, float* __restrict__ out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= t.cap_obj) return;
    const int n = min(max(t.state[0], 0), t.cap_obj);
    double sum = 0.0;
    int count = 0;
    if (row < n) {
        const int nv = min(max(t.nviews[row], 0), t.cap_views);
        for (int k = 0; k < nv; k++) {
            const size_t slot = (size_t)row * t.cap_views + k;
            double P[12], ob[4];
            for (int i = 0; i < 12; i++) P[i] = t.view_P34[slot * 12 + i];
            for (int i = 0; i < 4; i++) ob[i] = t.view_bbox[slot * 4 + i];
            Proj pr;
            project_row(t.axes + 3 * row, t.R + 9 * row, t.center + 3 * row, P, pr);
            const double iou = iou4(ob, pr.bbox);
            if (iou > 0.0) sum = sum + iou, count++;
        }
    }
    out[row] = count ? (float)(sum / (double)count) : 0.f;
}

ObjTable make_table(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* cat, int32_t* uid, int32_t* nviews,
                    float* view_P34, float* view_bbox, int32_t* state) {
    ObjTable t;
    t.cap_obj = cap_obj, t.cap_views = cap_views, t.axes = axes, t.R = R, t.center = center, t.cat = cat, t.uid = uid, t.nviews = nviews;
    t.view_P34 = view_P34, t.view_bbox = view_bbox, t.state = state;
    return t;
}

}  // namespace

static int dqo_launch_objmap_frame(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* cat, int32_t* uid, int32_t* nviews,
                                   float* view_P34, float* view_bbox, int32_t* state, int M, const float* det_bbox, const float* det_ellipse,
                                   const int32_t* det_cat, const float* det_score, const float* depth, const float* K, const float* Rt, int W, int H,
                                   int frame_id, uint64_t seed, int32_t* det_fate, int32_t* det_row, float* det_depth, uint8_t* opt_flag,
                                   int32_t* frame_header, hipStream_t s) {
    const ObjTable t = make_table(cap_obj, cap_views, axes, R, center, cat, uid, nviews, view_P34, view_bbox, state);
    ObjFrame f;
    f.M = M, f.W = W, f.H = H, f.frame_id = frame_id, f.seed = seed, f.bbox = det_bbox, f.ellipse = det_ellipse, f.score = det_score;
    f.depth = depth, f.K = K, f.Rt = Rt, f.cat = det_cat, f.fate = det_fate, f.row = det_row, f.det_depth = det_depth, f.opt_flag = opt_flag;
    f.header = frame_header;
    DQO_LAUNCH("objmap_frame_kernel", objmap_frame_kernel, dim3(1), dim3(OBJ_BLOCK), s, t, f);
    return DQO_OK;
}

static int dqo_launch_objmap_optimize(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* uid, int32_t* nviews,
                                      float* view_P34, float* view_bbox, int32_t* state, const uint8_t* opt_flag, int frame_id, uint64_t seed,
                                      float* loss_hist, hipStream_t s) {
    const ObjTable t = make_table(cap_obj, cap_views, axes, R, center, nullptr, uid, nviews, view_P34, view_bbox, state);
    DQO_LAUNCH("objmap_optimize_kernel", objmap_optimize_kernel, dim3((cap_obj + 63) / 64), dim3(64), s, t, opt_flag, frame_id, seed, loss_hist);
    return DQO_OK;
}

static int dqo_launch_objmap_mean_iou(int cap_obj, int cap_views, float* axes, float* R, float* center, int32_t* nviews, float* view_P34,
                                      float* view_bbox, int32_t* state, float* mean_iou, hipStream_t s) {
    const ObjTable t = make_table(cap_obj, cap_views, axes, R, center, nullptr, nullptr, nviews, view_P34, view_bbox, state);
    DQO_LAUNCH("objmap_mean_iou_kernel", objmap_mean_iou_kernel, dim3((cap_obj + 63) / 64), dim3(64), s, t, mean_iou);
    return DQO_OK;
}

// ---- entry points (include/dqo_raster.h): size queries, argument validation, the call ----
extern "C" {

// the object table's capacities: a row per lane of the one workgroup, a detection per lane of its first wave, room for a covering
// replacement's doubled observation; the observation slots stay indexable with int
static bool objmap_caps_ok(int32_t cap_obj, int32_t cap_views) {
    return cap_obj >= 1 && cap_obj <= 1024 && cap_views >= 2 && (int64_t)cap_obj * cap_views * 12 <= (int64_t)0x7fffffff;
}

DQO_API int dqo_objmap_frame(int32_t cap_obj, int32_t cap_views, int32_t cap_det, float* obj_axes, float* obj_R, float* obj_center,
                             int32_t* obj_cat, int32_t* obj_uid, int32_t* obj_nviews, float* view_P34, float* view_bbox, int32_t* state,
                             int32_t M, const float* det_bbox, const float* det_ellipse, const int32_t* det_cat, const float* det_score,
                             const float* depth, const float* K, const float* Rt, int32_t W, int32_t H, int32_t frame_id, uint64_t seed,
                             int32_t* det_fate, int32_t* det_row, float* det_depth, uint8_t* opt_flag, int32_t* frame_header, void* stream) {
    DQO_CHECK_ARG(objmap_caps_ok(cap_obj, cap_views), "bad capacities: cap_obj %d (1 to 1024), cap_views %d (2 or more)", cap_obj, cap_views);
    DQO_CHECK_ARG(cap_det >= 1 && cap_det <= 64, "bad capacity: cap_det %d (1 to 64)", cap_det);
    DQO_CHECK_ARG(M >= 1 && M <= cap_det, "bad detection count %d: 1 to cap_det = %d", M, cap_det);
    DQO_CHECK_ARG(W >= 1 && H >= 1 && (int64_t)W * H <= (int64_t)0x7fffffff, "bad image size %d x %d", W, H);
    DQO_CHECK_ARG(obj_axes && obj_R && obj_center && obj_cat && obj_uid && obj_nviews && view_P34 && view_bbox && state, "null pointer (table)");
    DQO_CHECK_ARG(det_bbox && det_ellipse && det_cat && det_score && depth && K && Rt, "null pointer (frame)");
    DQO_CHECK_ARG(det_fate && det_row && det_depth && opt_flag && frame_header, "null pointer (outputs)");
    return dqo_launch_objmap_frame(cap_obj, cap_views, obj_axes, obj_R, obj_center, obj_cat, obj_uid, obj_nviews, view_P34, view_bbox, state, M,
                                   det_bbox, det_ellipse, det_cat, det_score, depth, K, Rt, W, H, frame_id, seed, det_fate, det_row, det_depth,
                                   opt_flag, frame_header, (hipStream_t)stream);
}

DQO_API int dqo_objmap_optimize(int32_t cap_obj, int32_t cap_views, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_uid,
                                int32_t* obj_nviews, float* view_P34, float* view_bbox, int32_t* state, const uint8_t* opt_flag,
                                int32_t frame_id, uint64_t seed, float* loss_hist, void* stream) {
    DQO_CHECK_ARG(objmap_caps_ok(cap_obj, cap_views), "bad capacities: cap_obj %d (1 to 1024), cap_views %d (2 or more)", cap_obj, cap_views);
    DQO_CHECK_ARG(obj_axes && obj_R && obj_center && obj_uid && obj_nviews && view_P34 && view_bbox && state && opt_flag, "null pointer");
    return dqo_launch_objmap_optimize(cap_obj, cap_views, obj_axes, obj_R, obj_center, obj_uid, obj_nviews, view_P34, view_bbox, state, opt_flag,
                                      frame_id, seed, loss_hist, (hipStream_t)stream);
}

DQO_API int dqo_objmap_mean_iou(int32_t cap_obj, int32_t cap_views, float* obj_axes, float* obj_R, float* obj_center, int32_t* obj_nviews,
                                float* view_P34, float* view_bbox, int32_t* state, float* mean_iou, void* stream) {
    DQO_CHECK_ARG(objmap_caps_ok(cap_obj, cap_views), "bad capacities: cap_obj %d (1 to 1024), cap_views %d (2 or more)", cap_obj, cap_views);
    DQO_CHECK_ARG(obj_axes && obj_R && obj_center && obj_nviews && view_P34 && view_bbox && state && mean_iou, "null pointer");
    return dqo_launch_objmap_mean_iou(cap_obj, cap_views, obj_axes, obj_R, obj_center, obj_nviews, view_P34, view_bbox, state, mean_iou,
                                      (hipStream_t)stream);
}

}  // extern "C"
