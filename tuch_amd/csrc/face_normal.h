// The face normal of the admissibility rules and the vertex normal summed from it: one copy of each fixed float32
// sequence for cp_admissible and the cones (closest_point.hip), vertex_normals_kernel (vertex_normals.hip) and
// pc_fit_kernel<true> (point_cloud.hip).  Contraction is switched off inside each body, so the sequences are the same
// whatever mode the including file is in.
#pragma once
#include "common.h"

// The face normal of the admissibility rule: m = (b - a) x (c - a), one subtraction per component, each component of the
// product as (x y) - (z w), every operation rounded to float32 on its own.  t: the corners a, b, c, nine floats.
static __device__ __forceinline__ void cp_face_normal(const float* __restrict__ t, float& mx, float& my, float& mz)
{
#pragma clang fp contract(off)
    const float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
    const float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
    mx = (e1y * e2z) - (e1z * e2y);
    my = (e1z * e2x) - (e1x * e2z);
    mz = (e1x * e2y) - (e1y * e2x);
}

// Normal cones (closest_point.hip, file header "The cones", has the derivation of the classes and of the margin; the
// block cones of point_cloud.hip are the same record over a block's point normals).  cone = axis.xyz, cos beta,
// sin beta, usable (> 0), the smallest and the largest squared length of the normals it covers.
constexpr int kCpCone = 8;                          // floats per normal cone
constexpr float kCpConeMargin = 256.0f * 5.9604645e-8f;   // 256 * 2^-24, absolute, on cosines
constexpr float kCpSaneLo = 1e-30f, kCpSaneHi = 1e30f;    // |m|^2 of a covered normal inside: its square root and unit vector are sound
constexpr float kCpNormalLo = 1e-20f, kCpNormalHi = 1e20f; // |n|^2 of the lane inside: |A x n|^2 neither overflows nor underflows
constexpr float kCpPairLo = 1e-24f, kCpPairHi = 1e24f;    // |m|^2 |n|^2 inside: no under- or overflow that matters in the rule

// A cone against one lane's normal n with inv = 1 / |n|: 0 mixed, 1 wholly admissible, 2 wholly inadmissible.
static __device__ __forceinline__ int cp_cone_class(const float* __restrict__ cone, float nx, float ny, float nz, float inv, float c)
{
#pragma clang fp contract(fast)
    const float ax = cone[0], ay = cone[1], az = cone[2], cb = cone[3], sb = cone[4];
    const float ca = (ax * nx + ay * ny + az * nz) * inv;
    const float wx = ay * nz - az * ny, wy = az * nx - ax * nz, wz = ax * ny - ay * nx;
    const float sa = __builtin_sqrtf(wx * wx + wy * wy + wz * wz) * inv;
    const float sum = ca * cb - sa * sb;            // cos(alpha + beta)
    const float dif = ca * cb + sa * sb;            // cos(alpha - beta)
    int cls = 0;
    if (ca > 0.0f && cb > 0.0f && sum >= c + kCpConeMargin) cls = 1;
    if (ca < cb - kCpConeMargin && dif <= c - kCpConeMargin) cls = 2;
    const float nn = nx * nx + ny * ny + nz * nz;
    return cone[5] > 0.0f && cone[6] * nn >= kCpPairLo && cone[7] * nn <= kCpPairHi ? cls : 0;
}

static __device__ __forceinline__ int vn_clamp(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

// The unnormalised, area-weighted normal of vertex v of the body whose rows are `body` [V][3] (tuch_vertex_normals in
// include/tuch_amd.h): u = ((0 + m_1) + m_2) + ... per component over the faces vf_ids[vf_off[v] .. vf_off[v + 1]) in
// that order, m of cp_face_normal.  vf_ids has 3 F entries; every table entry is clamped before it addresses anything.
static __device__ __forceinline__ void vn_vertex_normal(const float* __restrict__ body, const int32_t* __restrict__ faces,
                                                        const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_ids,
                                                        int V, int F, int v, float& ux, float& uy, float& uz)
{
#pragma clang fp contract(off)
    const int from = vn_clamp(vf_off[v], 0, 3 * F), to = vn_clamp(vf_off[v + 1], from, 3 * F);
    ux = 0.0f; uy = 0.0f; uz = 0.0f;
    for (int j = from; j < to; ++j) {
        const int32_t* f = faces + (size_t)vn_clamp(vf_ids[j], 0, F - 1) * 3;
        float t[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* x = body + (size_t)vn_clamp(f[k], 0, V - 1) * 3;
            t[3 * k] = x[0]; t[3 * k + 1] = x[1]; t[3 * k + 2] = x[2];
        }
        float mx, my, mz;
        cp_face_normal(t, mx, my, mz);
        ux = ux + mx; uy = uy + my; uz = uz + mz;
    }
}
