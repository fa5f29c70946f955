// Pose evaluation on the device (the reference runs it on the host):
//   * procrustes_kernel: tuch/utils/pose_utils.py:28-92 (compute_similarity_transform{,_batch}, reconstruction_error),
//     a Python loop with one np.linalg.svd per body;
//   * pose_metrics_kernel: eval.py:158-195 and trainer.py:229-255 (joint regression, pelvis, joint map, MPJPE,
//     Procrustes-aligned MPJPE, mean vertex distance) for one batch in one launch.
// One wavefront per body.  Means, cross-covariance and variance are accumulated in float64 with a fixed lane
// assignment and a fixed butterfly, so a body's results do not depend on the batch around it; no atomics.
#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxR = 24;          // regressed joints (H36M: 17, SMPL: 24)
constexpr int kMaxJ = 64;          // mapped joints (one lane each in the MPJPE)
constexpr int kChunk = 256;        // regressor columns staged in LDS per step
constexpr int kBodiesPerBlock = 4; // pose_metrics_kernel: one wave per body, the staged regressor shared by four

// Sum over the 64 lanes; every lane gets the same bits (a + b == b + a at each butterfly level).
static __device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// Similarity transform of the reference (pose_utils.py:28-71) for one body, wave-uniform.  s1(n, d) / s2(n, d) read
// point n, coordinate d; hat(n, d, x) receives S1_hat (already rounded to the output type by the caller's functor,
// which returns the rounded value so the error uses what is stored, as the reference's float32 array does).
// err_rows_are_points: the error of reconstruction_error (sqrt over the last axis, mean over the one before) on an array
// whose rows are points (the [N,D] layout) or coordinates (the transposed [D,N] layout of pose_utils.py:35-39).
template <class L1, class L2, class H>
__device__ double procrustes_wave(L1 s1, L2 s2, int N, int D, bool err_rows_are_points, H hat)
{
    const int lane = threadIdx.x % kWave;
    // 1. means
    double m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0};
    for (int n = lane; n < N; n += kWave)
        for (int d = 0; d < D; ++d) { m1[d] += s1(n, d); m2[d] += s2(n, d); }
    for (int d = 0; d < D; ++d) { m1[d] = wave_sum(m1[d]) / N; m2[d] = wave_sum(m2[d]) / N; }
    // 2-3. var1 = sum |X1|^2, K = X1 X2^T (D x D)
    double var1 = 0.0, K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int n = lane; n < N; n += kWave) {
        double x1[3] = {0, 0, 0}, x2[3] = {0, 0, 0};
        for (int d = 0; d < D; ++d) { x1[d] = s1(n, d) - m1[d]; x2[d] = s2(n, d) - m2[d]; }
        for (int i = 0; i < D; ++i) {
            var1 += x1[i] * x1[i];
            for (int j = 0; j < D; ++j) K[i][j] += x1[i] * x2[j];
        }
    }
    var1 = wave_sum(var1);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) K[i][j] = wave_sum(K[i][j]);

    // 4. R = V Z U^T with K = U S V^T, Z = diag(1, .., sign(det(U V^T))): the rotation maximising tr(R K)
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (D == 2) {
        // closed form: R = [[c, -s], [s, c]] with (c, s) along (K00 + K11, K01 - K10)
        const double a = K[0][0] + K[1][1], b = K[0][1] - K[1][0];
        const double r = sqrt(a * a + b * b);
        const double c = r > 0.0 ? a / r : (a != a ? a : 1.0), s = r > 0.0 ? b / r : (a != a ? a : 0.0);
        R[0][0] = c; R[0][1] = -s; R[1][0] = s; R[1][1] = c;
    } else {
        // one-sided Jacobi on the columns of W = K V (V starts at I): at convergence w_i = sigma_i u_i
        double W[3][3], Vm[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) W[i][j] = K[i][j];
        for (int sweep = 0; sweep < 12; ++sweep) {
            bool rotated = false;
#pragma unroll
            for (int pq = 0; pq < 3; ++pq) {
                const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) { al += W[i][p] * W[i][p]; be += W[i][q] * W[i][q]; ga += W[i][p] * W[i][q]; }
                if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;       // orthogonal enough (or NaN: leave it)
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double wp = W[i][p], wq = W[i][q];
                    W[i][p] = c * wp - s * wq; W[i][q] = s * wp + c * wq;
                    const double vp = Vm[i][p], vq = Vm[i][q];
                    Vm[i][p] = c * vp - s * vq; Vm[i][q] = s * vp + c * vq;
                }
            }
            if (!rotated) break;
        }
        // singular values, sorted descending (selection of the order; ties keep the column order)
        double sg[3];
        for (int j = 0; j < 3; ++j) sg[j] = sqrt(W[0][j] * W[0][j] + W[1][j] * W[1][j] + W[2][j] * W[2][j]);
        int o[3] = {0, 1, 2};
        if (sg[o[1]] > sg[o[0]]) { const int x = o[0]; o[0] = o[1]; o[1] = x; }
        if (sg[o[2]] > sg[o[1]]) { const int x = o[1]; o[1] = o[2]; o[2] = x; }
        if (sg[o[1]] > sg[o[0]]) { const int x = o[0]; o[0] = o[1]; o[1] = x; }
        double u[3][3], v[3][3];                              // u[k], v[k]: k-th singular vectors
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 3; ++i) v[k][i] = Vm[i][o[k]];
        for (int i = 0; i < 3; ++i) u[0][i] = W[i][o[0]] / sg[o[0]];
        if (sg[o[1]] > 1e-12 * sg[o[0]]) {
            for (int i = 0; i < 3; ++i) u[1][i] = W[i][o[1]] / sg[o[1]];
        } else {
            // rank one (collinear S1): any unit vector orthogonal to u0; R u0 = v0 is all the result depends on
            const int a = fabs(u[0][0]) < fabs(u[0][1]) ? (fabs(u[0][0]) < fabs(u[0][2]) ? 0 : 2)
                                                         : (fabs(u[0][1]) < fabs(u[0][2]) ? 1 : 2);
            double e[3] = {0, 0, 0};
            e[a] = 1.0;
            const double dt = e[0] * u[0][0] + e[1] * u[0][1] + e[2] * u[0][2];
            for (int i = 0; i < 3; ++i) e[i] -= dt * u[0][i];
            const double nr = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            for (int i = 0; i < 3; ++i) u[1][i] = e[i] / nr;
        }
        // u2 = u0 x u1 (det U = +1).  Whatever the sign of the third left singular vector, z2 u2 is the same
        // (z2 = sign(det U det V) flips with it), so with det U = +1: z2 = sign(det V).
        u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
        u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
        u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
        const double detv = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1])
                          - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0])
                          + v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
        const double z2 = detv > 0 ? 1.0 : (detv < 0 ? -1.0 : detv);   // np.sign (NaN stays NaN)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = v[0][i] * u[0][j] + v[1][i] * u[1][j] + z2 * v[2][i] * u[2][j];
    }
    // 5. scale = tr(R K) / var1 (0 / 0 = NaN when all points of S1 coincide, as in the reference)
    double tr = 0.0;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) tr += R[i][j] * K[j][i];
    const double scale = tr / var1;
    // 6. t = mu2 - scale R mu1
    double t[3] = {0, 0, 0};
    for (int i = 0; i < D; ++i) {
        double rm = 0.0;
        for (int j = 0; j < D; ++j) rm += R[i][j] * m1[j];
        t[i] = m2[i] - scale * rm;
    }
    // 7. S1_hat and the error
    double e_pts = 0.0, e_crd[3] = {0, 0, 0};
    for (int n = lane; n < N; n += kWave) {
        double p[3] = {0, 0, 0};
        for (int d = 0; d < D; ++d) p[d] = s1(n, d);
        double sq = 0.0;
        for (int i = 0; i < D; ++i) {
            double y = 0.0;
            for (int j = 0; j < D; ++j) y += R[i][j] * p[j];
            const double h = hat(n, i, scale * y + t[i]);
            const double df = h - s2(n, i);
            sq += df * df;
            e_crd[i] += df * df;
        }
        e_pts += sqrt(sq);
    }
    if (err_rows_are_points) return wave_sum(e_pts) / N;
    double e = 0.0;
    for (int d = 0; d < D; ++d) e += sqrt(wave_sum(e_crd[d]));
    return e / D;
}

// S1, S2 [B, N, D] (coords_first = 0) or [B, D, N] (coords_first = 1, the reference's reading of a per-body matrix whose
// first axis is 2 or 3); S1_hat in the same layout (optional), err [B].
template <typename T>
__global__ __launch_bounds__(256) void procrustes_kernel(const T* __restrict__ S1, const T* __restrict__ S2, int B, int N,
                                                         int D, int coords_first, T* __restrict__ S1_hat, T* __restrict__ err)
{
    const int body = blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (body >= B) return;                    // whole waves: no barrier below
    const size_t base = (size_t)body * N * D;
    const int sn = coords_first ? 1 : D, sd = coords_first ? N : 1;
    const T* a = S1 + base;
    const T* b = S2 + base;
    T* h = S1_hat ? S1_hat + base : nullptr;
    auto s1 = [&](int n, int d) { return (double)a[n * sn + d * sd]; };
    auto s2 = [&](int n, int d) { return (double)b[n * sn + d * sd]; };
    auto hat = [&](int n, int d, double x) {
        const T y = (T)x;
        if (h) h[n * sn + d * sd] = y;
        return (double)y;
    };
    const double e = procrustes_wave(s1, s2, N, D, !coords_first, hat);
    if ((threadIdx.x % kWave) == 0) err[body] = (T)e;
}

// One wave per body, kBodiesPerBlock bodies per block.  The regressor [R,V] is read once per block: kChunk columns at a
// time are staged in LDS by the whole block and used by its four waves.  Lane l of a wave takes the vertices
// v = v0 + l + 64 k of each chunk and keeps R x 3 float partial sums for pred (and gt); after the last chunk the partials
// go through LDS and are summed in float64 column by column in lane order.  v2v is accumulated in the same pass.
__global__ __launch_bounds__(kBodiesPerBlock * kWave) void pose_metrics_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt_verts, const float* __restrict__ gt_joints,
    const float* __restrict__ reg, const int32_t* __restrict__ jmap, int B, int V, int R, int J, int pelvis,
    float* __restrict__ mpjpe, float* __restrict__ pa_mpjpe, float* __restrict__ v2v, float* __restrict__ joints_out)
{
    __shared__ float s_reg[kMaxR * kChunk];                              // 24 KB
    __shared__ float s_part[kBodiesPerBlock][kMaxR * 3][kWave + 1];      // 19.5 KB (+1: no bank conflicts on the writes)
    __shared__ double s_jp[kBodiesPerBlock][kMaxR * 3], s_jg[kBodiesPerBlock][kMaxR * 3];
    __shared__ double s_mp[kBodiesPerBlock][kMaxJ * 3], s_mg[kBodiesPerBlock][kMaxJ * 3];

    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int body = blockIdx.x * kBodiesPerBlock + w;
    const bool live = body < B;
    const bool has_gt_v = gt_verts != nullptr;
    const float* P = pred + (size_t)(live ? body : 0) * V * 3;
    const float* G = has_gt_v ? gt_verts + (size_t)(live ? body : 0) * V * 3 : nullptr;

    float ap[kMaxR][3], ag[kMaxR][3];
#pragma unroll
    for (int r = 0; r < kMaxR; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ap[r][c] = ag[r][c] = 0.f;
    double d_v2v = 0.0;

    for (int v0 = 0; v0 < V; v0 += kChunk) {
        const int cn = min(kChunk, V - v0);
        __syncthreads();                                                 // previous chunk consumed
        for (int i = threadIdx.x; i < R * kChunk; i += kBodiesPerBlock * kWave) {
            const int r = i / kChunk, c = i % kChunk;
            s_reg[i] = c < cn ? reg[(size_t)r * V + v0 + c] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        for (int c = lane; c < cn; c += kWave) {
            const size_t v = (size_t)(v0 + c) * 3;
            const float px = P[v], py = P[v + 1], pz = P[v + 2];
            float gx = 0.f, gy = 0.f, gz = 0.f;
            if (has_gt_v) {
                gx = G[v]; gy = G[v + 1]; gz = G[v + 2];
                const double dx = (double)px - gx, dy = (double)py - gy, dz = (double)pz - gz;
                d_v2v += sqrt(dx * dx + dy * dy + dz * dz);
            }
#pragma unroll
            for (int r = 0; r < kMaxR; ++r) {
                if (r < R) {
                    const float wr = s_reg[r * kChunk + c];
                    ap[r][0] = __builtin_fmaf(wr, px, ap[r][0]);
                    ap[r][1] = __builtin_fmaf(wr, py, ap[r][1]);
                    ap[r][2] = __builtin_fmaf(wr, pz, ap[r][2]);
                    if (has_gt_v) {
                        ag[r][0] = __builtin_fmaf(wr, gx, ag[r][0]);
                        ag[r][1] = __builtin_fmaf(wr, gy, ag[r][1]);
                        ag[r][2] = __builtin_fmaf(wr, gz, ag[r][2]);
                    }
                }
            }
        }
    }
    if (!live) return;                                                   // no block barrier below

    // lane partials -> float64 column sums in lane order (pred, then gt through the same buffer)
    const int RC = R * 3;
    for (int pass = 0; pass < (has_gt_v ? 2 : 1); ++pass) {
#pragma unroll
        for (int r = 0; r < kMaxR; ++r)
            if (r < R)
#pragma unroll
                for (int c = 0; c < 3; ++c) s_part[w][r * 3 + c][lane] = pass == 0 ? ap[r][c] : ag[r][c];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int j = lane; j < RC; j += kWave) {
            double s = 0.0;
            for (int l = 0; l < kWave; ++l) s += (double)s_part[w][j][l];
            (pass == 0 ? s_jp : s_jg)[w][j] = s;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (joints_out)
        for (int j = lane; j < RC; j += kWave) joints_out[(size_t)body * RC + j] = (float)s_jp[w][j];

    // pelvis (before the map, eval.py:177-186), map, MPJPE
    const double* jp = s_jp[w];
    const double* jg = s_jg[w];
    double pm = 0.0;
    if (lane < J) {
        const int m = jmap[lane];
        const bool ok = m >= 0 && m < R;
        for (int c = 0; c < 3; ++c) {
            const double p = ok ? jp[m * 3 + c] - jp[pelvis * 3 + c] : __builtin_nan("");
            const double g = has_gt_v ? (ok ? jg[m * 3 + c] - jg[pelvis * 3 + c] : __builtin_nan(""))
                                      : (double)gt_joints[((size_t)body * J + lane) * 3 + c];
            s_mp[w][lane * 3 + c] = p;
            s_mg[w][lane * 3 + c] = g;
            pm += (p - g) * (p - g);
        }
        pm = sqrt(pm);
    }
    pm = wave_sum(pm) / J;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // PA-MPJPE: the same similarity transform on the mapped joints (the reference's float32 arrays: S1_hat rounded)
    const double* mp = s_mp[w];
    const double* mg = s_mg[w];
    auto s1 = [&](int n, int d) { return mp[n * 3 + d]; };
    auto s2 = [&](int n, int d) { return mg[n * 3 + d]; };
    auto hat = [&](int, int, double x) { return (double)(float)x; };
    const double pa = procrustes_wave(s1, s2, J, 3, true, hat);
    const double vv = has_gt_v ? wave_sum(d_v2v) / V : 0.0;
    if (lane == 0) {
        mpjpe[body] = (float)pm;
        pa_mpjpe[body] = (float)pa;
        if (v2v && has_gt_v) v2v[body] = (float)vv;
    }
}

}  // namespace

extern "C" int tuch_procrustes(const void* S1, const void* S2, int B, int N, int D, int coords_first, int is_double,
                               void* S1_hat, void* err, void* stream)
{
    TUCH_REQUIRE(S1 && S2 && err, "tuch_procrustes: null pointer");
    TUCH_REQUIRE(B > 0 && N > 0 && (D == 2 || D == 3), "tuch_procrustes: bad sizes B=%d N=%d D=%d", B, N, D);
    const dim3 grid(ceil_div(B, 256 / kWave)), block(256);
    if (is_double)
        hipLaunchKernelGGL(procrustes_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)S1,
                           (const double*)S2, B, N, D, coords_first ? 1 : 0, (double*)S1_hat, (double*)err);
    else
        hipLaunchKernelGGL(procrustes_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)S1,
                           (const float*)S2, B, N, D, coords_first ? 1 : 0, (float*)S1_hat, (float*)err);
    return tuch_check_launch("tuch_procrustes");
}

extern "C" int tuch_pose_metrics(const float* pred_vertices, const float* gt_vertices, const float* gt_joints,
                                 const float* J_regressor, const int32_t* joint_map, int B, int V, int R, int J,
                                 int pelvis_index, float* mpjpe, float* pa_mpjpe, float* v2v, float* joints, void* stream)
{
    TUCH_REQUIRE(pred_vertices && J_regressor && joint_map && mpjpe && pa_mpjpe, "tuch_pose_metrics: null pointer");
    TUCH_REQUIRE((gt_vertices != nullptr) != (gt_joints != nullptr),
                 "tuch_pose_metrics: exactly one of gt_vertices / gt_joints");
    TUCH_REQUIRE(B > 0 && V > 0 && R > 0 && R <= kMaxR && J > 0 && J <= kMaxJ,
                 "tuch_pose_metrics: bad sizes B=%d V=%d R=%d (max %d) J=%d (max %d)", B, V, R, kMaxR, J, kMaxJ);
    TUCH_REQUIRE(pelvis_index >= 0 && pelvis_index < R, "tuch_pose_metrics: pelvis_index %d not in [0,%d)", pelvis_index, R);
    hipLaunchKernelGGL(pose_metrics_kernel, dim3(ceil_div(B, kBodiesPerBlock)), dim3(kBodiesPerBlock * kWave), 0,
                       (hipStream_t)stream, pred_vertices, gt_vertices, gt_joints, J_regressor, joint_map, B, V, R, J,
                       pelvis_index, mpjpe, pa_mpjpe, v2v, joints);
    return tuch_check_launch("tuch_pose_metrics");
}
