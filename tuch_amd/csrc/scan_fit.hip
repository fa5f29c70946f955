// The data term of a fit to unregistered points (tuch_scan_fit_terms, include/tuch_amd.h): for every real point of a scan
// the nearest point of the posed, translated mesh, a robust function of its squared distance, the bodies' weighted means,
// their total, and the unit gradients w.r.t. vertices, translation and points.
//
// Launches: the two of the closest-point search (closest_point.hip; the queries are points - transl, subtracted by the
// search itself), tuch_launch_zero_words on the gradient accumulator (a kernel, not a memset: a captured loop then holds
// kernel nodes only), scan_term_kernel, and in deterministic mode tuch_launch_fixed_to_float on the fixed-point sums: 4
// or 5.
//
//   scan_term_kernel   one point per thread, 256 per workgroup.  Every workgroup first adds up its body's weights
//                      (fit_body_sum: the normaliser, the same bits in every workgroup of the body, alone or in a batch),
//                      then g_q = w_q rho'(d2_q) / sum w (fit_rho) and r = (p - t) - c with c = sum_k bary_k x_k:
//                        grad_points = 2 g r,  rows of the winning face's corners += -2 g bary_k r  (fit_scatter_corners:
//                        64-bit fixed-point integer atomics in deterministic mode, float atomics otherwise),
//                        grad_transl = -sum_q 2 g r.
//                      The per-body sums (loss, normaliser, grad_transl) cross to the workgroup that arrives last through
//                      fit_reduce_tail and are added in chunk order there, the total in a fixed tree: no float atomics
//                      for them in either mode.  What is shared with the other fit terms is in fit_reduce.h; here are
//                      the loads, the per-point arithmetic and the launcher.
//
// A point of weight 0 is not computed from (it may be non-finite); neither is one the search found no face for (a body
// with non-finite vertices).  A body without weight (counts[b] = 0, or all weights 0) has loss 0 and zero gradient rows.
#include "fit_reduce.h"
#include "model.h"
#include "workspace.h"

namespace {

constexpr int kBlock = kFitBlock;

struct ScanLayout { size_t search, fixed, partial, total; };

ScanLayout scan_layout(const tuch_contact_model* m, int B, int Q, bool oriented)
{
    ScanLayout l;
    size_t o = 0;
    // (the search guards its own regions: its layout is recorded by its own scope at this offset)
    l.search = tuch_ws_take(o, tuch_closest_point_workspace_bytes(m, B, Q, oriented), false);
    l.fixed = tuch_ws_take(o, (size_t)B * m->V * 3 * sizeof(long long));
    l.partial = tuch_ws_take(o, (size_t)B * ceil_div(Q, kBlock) * kFitPart * sizeof(float));
    l.total = o;
    return l;
}

static __device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

template <bool kFixed>
__global__ __launch_bounds__(kBlock) void scan_term_kernel(
    const float* __restrict__ verts, const float* __restrict__ transl, const float* __restrict__ points,
    const int32_t* __restrict__ counts, const float* __restrict__ weights, const float* __restrict__ d2,
    const int32_t* __restrict__ face, const float* __restrict__ bary, const int32_t* __restrict__ faces, int B, int V, int F,
    int Q, int rho, float sigma2, float* partial, int* ticket, float* __restrict__ per_body, float* __restrict__ total,
    float* __restrict__ grad_points, float* __restrict__ grad_verts, long long* __restrict__ grad_fixed,
    float* __restrict__ grad_transl)
{
    __shared__ FitShared sh;
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    int count = Q;
    if (counts) {
        count = counts[b];
        count = count < 0 ? 0 : (count > Q ? Q : count);
    }
    // the normaliser: this body's weights
    float wsum = (float)count;
    if (weights) wsum = fit_body_sum(sh, count, [&](int i) { return weights[(size_t)b * Q + i]; });
    const int q = c * kBlock + t;
    float s = 0.0f, ex = 0.0f, ey = 0.0f, ez = 0.0f;
    if (q < count) {
        const size_t o = (size_t)b * Q + q;
        const float w = weights ? weights[o] : 1.0f;
        const int f = face[o];
        if (w != 0.0f && wsum != 0.0f && f >= 0 && f < F) {
            float value, slope;
            fit_rho(rho, sigma2, d2[o], value, slope);
            s = w * value;
            const float g2 = 2.0f * (w * slope / wsum);
            const float bw[3] = {bary[o * 3], bary[o * 3 + 1], bary[o * 3 + 2]};
            int vi[3];
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                vi[k] = clamp_index(faces[(size_t)f * 3 + k], V);
                const float* x = verts + ((size_t)b * V + vi[k]) * 3;
                cx = __builtin_fmaf(bw[k], x[0], cx); cy = __builtin_fmaf(bw[k], x[1], cy); cz = __builtin_fmaf(bw[k], x[2], cz);
            }
            // (the query as the search formed it: one subtraction per component)
            ex = g2 * ((points[o * 3] - transl[3 * b]) - cx);
            ey = g2 * ((points[o * 3 + 1] - transl[3 * b + 1]) - cy);
            ez = g2 * ((points[o * 3 + 2] - transl[3 * b + 2]) - cz);
            fit_scatter_corners<kFixed>(grad_verts, grad_fixed, (size_t)b * V, vi, bw, ex, ey, ez);
        }
    }
    if (grad_points && q < Q) {
        float* g = grad_points + ((size_t)b * Q + q) * 3;
        g[0] = ex; g[1] = ey; g[2] = ez;
    }
    fit_reduce_tail(sh, s, -ex, -ey, -ez, wsum, 1.0f, partial, ticket, B, per_body, total, grad_transl);
}

}  // namespace

extern "C" size_t tuch_scan_fit_workspace_bytes(const tuch_contact_model* m, int B, int Q, int oriented)
{
    if (!m || B <= 0 || Q <= 0) return 0;
    tuch_ws_scope scope(m->opt.canary != 0);
    return scan_layout(m, B, Q, oriented != 0).total;
}

extern "C" int tuch_scan_fit_terms(const tuch_contact_model* m, const float* verts, const float* transl, const float* points,
                                   const float* normals, float max_angle_cos, const int32_t* counts, const float* weights,
                                   const int32_t* hint, int B, int Q, int rho, float sigma, float* d2, int32_t* face,
                                   float* bary, int* ticket, float* per_body, float* total, float* grad_verts,
                                   float* grad_transl, float* grad_points, void* workspace, size_t workspace_bytes,
                                   void* stream)
{
    const char* name = "tuch_scan_fit_terms";
    int rc = tuch_cp_check_cos(name, normals, max_angle_cos);
    if (rc != TUCH_OK) return rc;
    TUCH_REQUIRE(m && verts && transl && points && d2 && face && bary && ticket && per_body && total && grad_verts && grad_transl,
                 "%s: null pointer", name);
    TUCH_REQUIRE(B > 0 && B <= 65535 && Q > 0 && (long long)B * ceil_div(Q, kBlock) < (1ll << 30), "%s: bad sizes B=%d Q=%d", name,
                 B, Q);
    TUCH_REQUIRE(rho == TUCH_SCAN_RHO_SQUARED || rho == TUCH_SCAN_RHO_DISTANCE || (rho == TUCH_SCAN_RHO_GMOF && sigma > 0.0f),
                 "%s: rho %d (0 squared, 1 distance, 2 gmof with sigma > 0; sigma = %g)", name, rho, (double)sigma);
    const bool oriented = normals != nullptr;
    const size_t need = tuch_scan_fit_workspace_bytes(m, B, Q, oriented);
    if (!workspace || workspace_bytes < need) {
        tuch_set_error("%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
        return TUCH_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    tuch_ws_scope scope(m->opt.canary != 0);
    const ScanLayout l = scope.record(0, [&] { return scan_layout(m, B, Q, oriented); });
    scope.arm(workspace, m->canary_hits, s);
    rc = tuch_cp_search(name, m, verts, points, transl, normals, max_angle_cos, counts, hint, B, Q, d2, face, bary,
                        (char*)workspace + l.search, tuch_closest_point_workspace_bytes(m, B, Q, oriented), stream);
    if (rc != TUCH_OK) return rc;
    long long* fixed = (long long*)((char*)workspace + l.fixed);
    float* partial = (float*)((char*)workspace + l.partial);
    const bool det = tuch_deterministic() != 0;
    const size_t n = (size_t)B * m->V * 3;
    tuch_launch_zero_words(det ? (void*)fixed : (void*)grad_verts, det ? 2 * n : n, s);
    const dim3 grid(ceil_div(Q, kBlock), B);
    const float sigma2 = sigma * sigma;
    if (det) {
        hipLaunchKernelGGL(scan_term_kernel<true>, grid, dim3(kBlock), 0, s, verts, transl, points, counts, weights,
                           (const float*)d2, (const int32_t*)face, (const float*)bary, (const int32_t*)m->faces, B, m->V, m->F,
                           Q, rho, sigma2, partial, ticket, per_body, total, grad_points, (float*)nullptr, fixed, grad_transl);
        tuch_launch_fixed_to_float(fixed, grad_verts, n, s);
    } else {
        hipLaunchKernelGGL(scan_term_kernel<false>, grid, dim3(kBlock), 0, s, verts, transl, points, counts, weights,
                           (const float*)d2, (const int32_t*)face, (const float*)bary, (const int32_t*)m->faces, B, m->V, m->F,
                           Q, rho, sigma2, partial, ticket, per_body, total, grad_points, grad_verts, (long long*)nullptr,
                           grad_transl);
    }
    return tuch_check_launch(name);
}
