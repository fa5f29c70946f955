// Posed vertex normals (tuch_vertex_normals, include/tuch_amd.h): for every vertex the sum of the normals
// m = (b - a) x (c - a) of the faces around it -- the area-weighted normal -- in the order of the vertex -> faces table
// (ops.vertex_face_table: ascending face ids), optionally normalised.
//
// The rule is one fixed float32 sequence (face_normal.h: cp_face_normal, the m of tuch_closest_point's
// admissibility rule, and vn_vertex_normal, the left-to-right sum from 0), nothing fused.  normalize != 0 divides by
// sqrt(uu), uu = (ux ux + uy uy) + uz uz, and writes a zero row where uu is 0 or not finite (a vertex without faces,
// faces without area, a non-finite corner).  One lane owns one row: it reads the corners of its vertex's faces and
// writes three floats; no atomics, no cross-lane traffic, no workspace.  So a vertex has the same bits alone or in any
// batch, eager or replayed, and a body that holds NaN changes no other body's bits (a lane reads rows of its own body
// only).  Every table entry is clamped before it addresses anything.  There are no gradients.
//
// Cost.  A vertex of a closed triangle mesh has six faces on average: 6 x 9 floats gathered from rows its neighbours
// read too (SMPL: 83 KB of vertices per body, resident in L2), 3 floats written.  The launch is bound by its latency
// at SMPL's size (B x 6890 lanes); pc_fit_kernel<true> (point_cloud.hip) calls vn_vertex_normal itself and needs no
// launch of this kernel.
#include "face_normal.h"

namespace {

constexpr int kVnBlock = 256;

__global__ __launch_bounds__(kVnBlock) void vertex_normals_kernel(const float* __restrict__ verts,
                                                                 const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ vf_off,
                                                                 const int32_t* __restrict__ vf_ids, int V, int F,
                                                                 int normalize, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int b = blockIdx.y, v = blockIdx.x * kVnBlock + threadIdx.x;
    if (v >= V) return;
    float ux, uy, uz;
    vn_vertex_normal(verts + (size_t)b * V * 3, faces, vf_off, vf_ids, V, F, v, ux, uy, uz);
    if (normalize) {
        const float uu = (ux * ux + uy * uy) + uz * uz;
        const bool known = uu > 0.0f && __builtin_isfinite(uu);
        const float len = __builtin_sqrtf(uu);
        ux = known ? ux / len : 0.0f; uy = known ? uy / len : 0.0f; uz = known ? uz / len : 0.0f;
    }
    float* o = out + ((size_t)b * V + v) * 3;
    o[0] = ux; o[1] = uy; o[2] = uz;
}

}  // namespace

extern "C" int tuch_vertex_normals(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_ids,
                                   int B, int V, int F, int normalize, float* out, void* stream)
{
    TUCH_REQUIRE(verts && faces && vf_off && vf_ids && out, "tuch_vertex_normals: null pointer");
    TUCH_REQUIRE(B > 0 && B <= 65535 && V > 0 && F > 0 && (long long)B * V < (1ll << 31) && (long long)F * 3 < (1ll << 31),
                 "tuch_vertex_normals: bad sizes B=%d V=%d F=%d", B, V, F);
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(ceil_div(V, kVnBlock), B), dim3(kVnBlock), 0, (hipStream_t)stream, verts,
                       faces, vf_off, vf_ids, V, F, normalize, out);
    return tuch_check_launch("tuch_vertex_normals");
}
