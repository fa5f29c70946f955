// Inside test by signed ray crossings on gfx950 -- the exterior flags of tuch/smplify/losses.py:81-82 and
// tuch/train/loss.py:260-262,297 (`winding_numbers(...).le(0.99)`) without summing solid angles.
//
// For a point p off a closed oriented mesh M the winding number w(p) = 1/(4 pi) sum_f Omega_f(p) is an INTEGER:
// the signed number of crossings of any ray from p with M (+1 where the ray leaves through a face along its
// outward normal, -1 where it enters).  That covers the HD points of loss.py:297 (1 mm off the surface).
// For a VERTEX v of M the reference's sum skips the faces around v (their terms are atan2(0,0) = 0,
// contact.py:105), i.e. it is the solid angle of M' = M minus star(v), a surface with the one-ring of v as its
// boundary.  Close M' with a fan S = {(a, r_j, r_j+1)} over the ring with an apex a = v + delta u, a != v: then
//     sum_{f in M'} Omega_f(v) + sum_{g in S} Omega_g(v) = 4 pi N,    N = signed ray crossings of M' u S from v,
// so   w_ref(v) = N - 1/(4 pi) sum_{g in S} Omega_g(v):  an integer from ~1.5 k cheap crossing tests (no sqrt, no
// atan) plus valence(v) ~ 6 solid angles -- instead of ~2.5 k solid-angle steps of the cluster-tree walk
// (winding.hip) and ~14 k of the flat walk.  Both fan terms depend on the DIRECTION u only (the solid-angle
// formula is homogeneous of degree 0 in every corner vector; a ray from the origin hits the triangle (delta u, B, C)
// iff its direction lies in the cone spanned by u, B, C), so delta never appears.
//
// Crossings are counted along ONE fixed direction for all queries, in sheared coordinates
//     x' = x - kx z,  y' = y - ky z,  z' = z        (ray = +z', i.e. direction (kx, ky, 1) in space)
// where a triangle is hit iff the origin of the query-relative (x', y') plane lies inside its projection and the
// hit is in front.  Edge functions e(P,Q) = fl(Px Qy) - fl(Py Qx) are evaluated WITHOUT fma: they are exactly
// antisymmetric, so two triangles sharing an edge always agree on which side of it the ray passes, and the
// ties e == 0 are broken by the lexicographic order of the endpoints (the rasteriser's top-left rule): every ray
// is assigned to exactly one of the triangles around an edge or a vertex -- the count is the exact integer
// winding number of the float-coordinate mesh.  The walk uses the model's cluster tree (cluster_tree.hip): a
// node is entered only if the ray of some query of the wavefront can meet its 9-slab volume; far nodes cost
// nothing (no boundary caps are needed: a ray that misses a node's volume crosses none of its faces).
//
// The result equals thresholding the reference's float sum wherever that sum is not within its own rounding
// noise (~1e-5) of the threshold; tests/test_gpu_contact.py compares the two on every fixture.
#include "common.h"
#include "model.h"
#include "workspace.h"
#include "tree_device.h"
#include <stdlib.h>

#pragma clang fp contract(off)      // edge functions must stay mul, mul, sub (exact antisymmetry)

namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr int kBlock = 256;
constexpr int kRayQueries = 64;               // one query per lane
constexpr float kShearX = 0.3217f, kShearY = 0.4331f;
// apex direction of the closing fan (any direction that is not +-ray and not in a ring face's plane)
constexpr float kFanX = 0.8191f, kFanY = 0.3467f, kFanZ = 0.4571f;
constexpr int kSlabs = 9;
constexpr int kSlabStride = 10;               // as winding.hip: node = [lo[10], hi[10]]
constexpr int kNearSlabs = 13;                // of the 18 slab values of a leaf, those the near test uses

struct RayElem { float x, y, z, sign; };      // sheared position of a strip vertex; `sign` holds the model's word for the
                                              // element (tree_sign_word): bits 0-23 the orientation of the triangle it
                                              // closes as the INTEGER +1 / -1 / 0, bits 24-31 the segments that list it

__device__ __forceinline__ float shear_x(float x, float z) { return __builtin_fmaf(-kShearX, z, x); }
__device__ __forceinline__ float shear_y(float y, float z) { return __builtin_fmaf(-kShearY, z, y); }

// ---- per call: sheared leaf strips + node slabs ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ray_stream_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ vidx, const float* __restrict__ sign,
    int V, int L, int Lpad, RayElem* __restrict__ out, uint4* __restrict__ zeroed, size_t zeroed_n)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    // also clears the counters of the kernels that follow (a separate 6 MB fill in front of the chain was 12 us)
    for (size_t g = ((size_t)b * gridDim.x + blockIdx.x) * kBlock + threadIdx.x; g < zeroed_n;
         g += (size_t)gridDim.x * gridDim.y * kBlock)
        zeroed[g] = make_uint4(0u, 0u, 0u, 0u);
    if (p >= Lpad) return;
    RayElem e = {0.f, 0.f, 0.f, 0.f};
    if (p < L) {
        const float* c = verts + ((size_t)b * V + vidx[p]) * 3;
        e.x = shear_x(c[0], c[2]); e.y = shear_y(c[1], c[2]); e.z = c[2]; e.sign = sign[p];
    }
    out[(size_t)b * Lpad + p] = e;
}

__device__ __forceinline__ void slab_project(float x, float y, float z, float (&p)[kSlabs])
{
    p[0] = x; p[1] = y; p[2] = z;
    p[3] = x + y; p[4] = x - y; p[5] = x + z; p[6] = x - z; p[7] = y + z; p[8] = y - z;
}

// minimum over the 16 lanes of a DPP row, left in every lane: quad swaps, then the two mirror controls -- single VALU
// instructions, no LDS crossbar (a 64-lane shuffle reduction of the 18 slab values was ~200 instructions per leaf)
template <int kCtrl>
__device__ __forceinline__ float dpp_move(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_min(float v)
{
    v = fminf(v, dpp_move<0xB1>(v));        // quad_perm [1,0,3,2]
    v = fminf(v, dpp_move<0x4E>(v));        // quad_perm [2,3,0,1]
    v = fminf(v, dpp_move<0x141>(v));       // row_half_mirror
    v = fminf(v, dpp_move<0x140>(v));       // row_mirror
    return v;
}

// slabs of every leaf in sheared coordinates, 16 lanes per (leaf, body): a leaf strip is a few dozen elements, so a
// whole wavefront per leaf was mostly idle lanes behind four dependent rounds of loads; widened by a few ulps so that
// a ray decided by the float edge functions to pass on the leaf's side of a shared edge can never test as missing it
// kPose: the kernel also WRITES the sheared strip (each 16-lane group poses the run of its own leaf; the leaves' runs
// tile the stream, checked at model creation) and clears the counters of the kernels that follow -- ray_stream_kernel's
// work, without a launch of its own ahead of this one on the step's serial chain.
// ---- the near test's numbers: signed 16-bit fixed point ------------------------------------------------------------------
// Both sides of the near test (ray_near_kernel) -- a leaf's 13 bounds and a ray's nine values, all relative to the body's
// reference point -- are levels k / kNearScale, k in [-32768, 32767]: steps of 2^-13 m over [-4 m, 4 m).  (Half precision
// on the bounds alone steps by 2^-10 m beyond 1 m from the reference point; tools/diag/near_encode_sim.py counts the pairs
// listed with either)  up: the smallest level >= v, otherwise the largest level <= v; where no such level
// exists, and for NaN, the end of the range on that side: +32767 rounding up, -32768 rounding down.  A number that is
// rounded UP is only ever the right-hand side of a `bound > value` rejection (an upper bound, or a ray's value set against a
// lower bound), one rounded DOWN only the left-hand side -- so those two codes can never reject.  The conversion is
// monotone: v <= w implies near_encode(v) <= near_encode(w) in either direction (NaN aside).
constexpr float kNearScale = 8192.0f;
constexpr int kNearMin = -32768, kNearMax = 32767;
__host__ __device__ __forceinline__ int near_encode(float v, bool up)
{
    const float t = v * kNearScale;                 // exact (a power of two), +-inf beyond the float range
    if (up) {
        const float c = __builtin_ceilf(t);
        return !(c <= (float)kNearMax) ? kNearMax : c < (float)kNearMin ? kNearMin : (int)c;       // NaN: kNearMax
    }
    const float c = __builtin_floorf(t);
    return !(c >= (float)kNearMin) ? kNearMin : c > (float)kNearMax ? kNearMax : (int)c;           // NaN: kNearMin
}
__host__ __device__ __forceinline__ uint32_t near_pack(int lo_half, int hi_half)
{
    return ((uint32_t)lo_half & 0xffffu) | (uint32_t)hi_half << 16;
}
// where the tables of one call's `bounds` region start (floats): [B][13][L] | records [B][L][8 dwords] | centres [B][4]
__device__ __host__ __forceinline__ size_t near_records_at(int B, int L) { return (size_t)B * kNearSlabs * L; }
__device__ __host__ __forceinline__ size_t near_centres_at(int B, int L) { return near_records_at(B, L) + (size_t)B * L * 8; }

// ---- the crossing walk's filter box of one strip element -------------------------------------------------------------
// (x'min, x'max, y'min, y'max) of the triangle (p0, p1, p2) the element closes, in the sheared frame and in the stream's
// own floats, widened by kBoxPad.  The walk tests a (ray, element) pair exactly only if the ray's origin (q'x, q'y) lies
// in the box (inclusive); see the walk's header (above ray_exact) for why a pair outside it can never count.  Three kinds of element get a box
// that decides nothing:
//   priming elements (no triangle)                 : the empty box (+inf, -inf, +inf, -inf);
//   a corner beyond kBoxRange in x' or y', or NaN  : the full box (-inf, +inf, -inf, +inf);
//   slivers in projection                          : the full box -- the projected triangle's smallest altitude is at
//     most kBoxSliver (2 area <= kBoxSliver * sqrt 2 * longest edge in the max norm, which is >= the Euclidean edge / sqrt 2).
constexpr float kBoxRange = 16.0f;                      // |x'|, |y'| of corners AND origins the filter decides for
constexpr float kBoxPad = 0x1p-13f;                     // 0.12 mm; >> ulp(kBoxRange) = 2^-19, the rounding of min - pad
constexpr float kBoxSliver = 0x1p-14f;                  // = 2^-18 kBoxRange, see the walk's header
__device__ __forceinline__ float4 ray_elem_box(const RayElem& p0, const RayElem& p1, const RayElem& p2)
{
    const float inf = __builtin_inff();
    if ((__float_as_int(p2.sign) & 0xffffff) == 0) return make_float4(inf, -inf, inf, -inf);
    const float x0 = fminf(fminf(p0.x, p1.x), p2.x), x1 = fmaxf(fmaxf(p0.x, p1.x), p2.x);
    const float y0 = fminf(fminf(p0.y, p1.y), p2.y), y1 = fmaxf(fmaxf(p0.y, p1.y), p2.y);
    const float ax = p1.x - p0.x, ay = p1.y - p0.y, bx = p2.x - p0.x, by = p2.y - p0.y;
    const float area2 = fabsf(ax * by - ay * bx);
    const float edge = fmaxf(fmaxf(x1 - x0, y1 - y0), 0.0f);      // longest edge in the max norm = the larger box side
    const bool in_range = fmaxf(fmaxf(fabsf(x0), fabsf(x1)), fmaxf(fabsf(y0), fabsf(y1))) <= kBoxRange;
    const bool solid = area2 > kBoxSliver * 1.4142137f * edge;     // false when a coordinate is NaN (area2 is NaN then)
    if (!in_range || !solid) return make_float4(-inf, inf, -inf, inf);
    return make_float4(x0 - kBoxPad, x1 + kBoxPad, y0 - kBoxPad, y1 + kBoxPad);
}

template <bool kPose>
__global__ __launch_bounds__(kBoundsBlock) void ray_leaf_bounds_kernel(
    const RayElem* __restrict__ stream, int T, const TreeNode* __restrict__ nodes, int N,
    const int32_t* __restrict__ height_off, const int32_t* __restrict__ height_nodes, float* __restrict__ bounds,
    const float* __restrict__ verts, const int32_t* __restrict__ vidx, const float* __restrict__ sign, int V, int Lexact,
    RayElem* __restrict__ stream_out, uint4* __restrict__ zeroed, size_t zeroed_n, float4* __restrict__ boxes, int keep_bounds)
{
    const int b = blockIdx.y;
    const RayElem* st = stream + (size_t)b * T;
    const int group = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const int i = height_off[0] + blockIdx.x * (kBoundsBlock / 16) + group;
    const bool real = i < height_off[1];                // all lanes stay: the DPP rows need them
    const int node = height_nodes[real ? i : height_off[0]];
    const int off = nodes[node].ex_off, len = real ? nodes[node].ex_len : 0;
    if (kPose) {
        for (size_t g = ((size_t)b * gridDim.x + blockIdx.x) * kBoundsBlock + threadIdx.x; g < zeroed_n;
             g += (size_t)gridDim.x * gridDim.y * kBoundsBlock)
            zeroed[g] = make_uint4(0u, 0u, 0u, 0u);
        if (blockIdx.x == 0)                            // the padding behind the last run (three readable elements past the end)
            for (int p = Lexact + (int)threadIdx.x; p < T; p += kBoundsBlock) stream_out[(size_t)b * T + p] = RayElem{0.f, 0.f, 0.f, 0.f};
    }
    if (blockIdx.x == 0)                                // ... and its boxes: empty (the walk reads three boxes ahead)
        for (int p = Lexact + (int)threadIdx.x; p < T; p += kBoundsBlock)
            boxes[(size_t)b * T + p] = make_float4(__builtin_inff(), -__builtin_inff(), __builtin_inff(), -__builtin_inff());
    auto posed = [&](int p) {                           // element p of the posed, sheared stream: the same floats either way
        RayElem e;
        if (kPose) {
            const float* c = verts + ((size_t)b * V + vidx[p]) * 3;
            e.x = shear_x(c[0], c[2]); e.y = shear_y(c[1], c[2]); e.z = c[2]; e.sign = sign[p];
        } else {
            e = st[p];
        }
        return e;
    };
    float lo[kSlabs], nhi[kSlabs];                      // minima of the projections and of their negatives
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) { lo[k] = 3.0e38f; nhi[k] = 3.0e38f; }
    for (int p = sub; p < len; p += 16) {
        const RayElem e = posed(off + p);
        if (kPose) stream_out[(size_t)b * T + off + p] = e;
        // the box of the triangle the element closes (its two predecessors lie in the same run: a run starts with the two
        // priming elements of its first strip, whose boxes are empty whatever is read for them)
        boxes[(size_t)b * T + off + p] = ray_elem_box(posed(off + max(p - 2, 0)), posed(off + max(p - 1, 0)), e);
        float pr[kSlabs];
        slab_project(e.x, e.y, e.z, pr);
#pragma unroll
        for (int k = 0; k < kSlabs; ++k) { lo[k] = fminf(lo[k], pr[k]); nhi[k] = fminf(nhi[k], -pr[k]); }
    }
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) { lo[k] = row_min(lo[k]); nhi[k] = row_min(nhi[k]); }
    if (real && sub == 0) {
        // the 13 slab values the near test uses, padded for the roundings of the projections (round 2-3: also stored in
        // single precision, one array per value over the leaves; since round 4 ray_near_kernel reads the records alone)
        const int L = height_off[1] - height_off[0], leaf = i - height_off[0];
        float lo_p[kSlabs], hi_p[kSlabs];
#pragma unroll
        for (int k = 0; k < kSlabs; ++k) {
            const float hi = -nhi[k];
            const float pad = 4e-7f * fmaxf(fabsf(lo[k]), fabsf(hi)) + 1e-9f;
            lo_p[k] = lo[k] - pad;
            hi_p[k] = hi + pad;
        }
        // ... as the 32-byte RECORD both stages of the near test read: 16-bit fixed point (near_encode), relative to a
        // reference point of the body (the first element of its strip, so that the numbers stay small wherever the body
        // stands), lower bounds rounded down and upper bounds up after a pad for the roundings of the subtraction.
        float c[3];
        if (kPose) {
            const float* c0 = verts + ((size_t)b * V + vidx[0]) * 3;
            c[0] = shear_x(c0[0], c0[2]); c[1] = shear_y(c0[1], c0[2]); c[2] = c0[2];
        } else {
            const RayElem e0 = st[0];
            c[0] = e0.x; c[1] = e0.y; c[2] = e0.z;
        }
        float pc[kSlabs];
        slab_project(c[0], c[1], c[2], pc);
        float lo_r[kSlabs], hi_r[kSlabs];
        int lo_h[kSlabs], hi_h[kSlabs];
#pragma unroll
        for (int k = 0; k < kSlabs; ++k) {
            const float pad = 4e-6f * (fabsf(lo_p[k]) + fabsf(hi_p[k]) + fabsf(pc[k])) + 1e-7f;
            lo_r[k] = lo_p[k] - pc[k] - pad;
            hi_r[k] = hi_p[k] - pc[k] + pad;
            lo_h[k] = near_encode(lo_r[k], false);
            hi_h[k] = near_encode(hi_r[k], true);
        }
        uint4* r = reinterpret_cast<uint4*>(bounds + near_records_at(gridDim.y, L)) + ((size_t)b * L + leaf) * 2;
        r[0] = make_uint4(near_pack(lo_h[0], lo_h[1]), near_pack(lo_h[3], lo_h[4]), near_pack(lo_h[6], lo_h[8]), near_pack(hi_h[0], hi_h[1]));
        r[1] = make_uint4(near_pack(hi_h[2], hi_h[3]), near_pack(hi_h[4], hi_h[5]), near_pack(hi_h[7], leaf), (uint32_t)node);  // + who it is
        if (keep_bounds) {      // tuch_ray_near_debug: the 13 single-precision bounds behind the record, in the order of its halves
            float* o = bounds + ((size_t)b * kNearSlabs) * L + leaf;
            const float v[kNearSlabs] = {lo_r[0], lo_r[1], lo_r[3], lo_r[4], lo_r[6], lo_r[8], hi_r[0], hi_r[1], hi_r[2], hi_r[3], hi_r[4], hi_r[5], hi_r[7]};
#pragma unroll
            for (int k = 0; k < kNearSlabs; ++k) o[(size_t)k * L] = v[k];
        }
        if (leaf == 0) *reinterpret_cast<float4*>(bounds + near_centres_at(gridDim.y, L) + (size_t)b * 4) = make_float4(c[0], c[1], c[2], 0.f);
    }
}

// ---- crossing test --------------------------------------------------------------------------------------------
struct P3 { float x, y, z; };

__device__ __forceinline__ float edge_fn(const P3& p, const P3& q) { return p.x * q.y - p.y * q.x; }   // no fma (pragma)

// tie-break for e(P,Q) == 0: is the origin "left of or on" the directed edge P -> Q?  Lexicographic order of the
// endpoints; exactly one of (P,Q), (Q,P) answers true.
__device__ __forceinline__ bool left_of(float e, const P3& p, const P3& q)
{
    return e > 0.0f || (e == 0.0f && (p.x < q.x || (p.x == q.x && p.y < q.y)));
}

// signed crossing of the +z ray from the origin with the triangle (a, b, c) given relative to the query;
// ea = e(b,c), eb = e(c,a), ec = e(a,b) (edge opposite each corner).  +1: the ray leaves through the front of
// (a,b,c) (det(a,b,c) > 0), -1: enters, 0: no hit in front.
__device__ __forceinline__ int crossing(const P3& a, const P3& b, const P3& c, float ea, float eb, float ec)
{
    const bool la = left_of(ea, b, c), lb = left_of(eb, c, a), lc = left_of(ec, a, b);
    const bool pos = la && lb && lc, neg = !la && !lb && !lc;
    if (!(pos || neg)) return 0;
    const float numz = ea * a.z + eb * b.z + ec * c.z;          // = det(a,b,c): sign of the crossing, and of the depth
    if (pos) return numz > 0.0f ? 1 : 0;
    return numz < 0.0f ? -1 : 0;
}

// the same through the branch-free generic form, the careful one only for lanes with an exact tie (wave-uniform test)
__device__ __forceinline__ int crossing_mostly_generic(const P3& a, const P3& b, const P3& c, float ea, float eb, float ec)
{
    const float numz = ea * a.z + eb * b.z + ec * c.z;
    const float mn = __builtin_fminf(__builtin_fminf(ea, eb), ec), mx = __builtin_fmaxf(__builtin_fmaxf(ea, eb), ec);
    int n = (int)(__builtin_fminf(mn, numz) > 0.0f) - (int)(__builtin_fmaxf(mx, numz) < 0.0f);
    const bool tie = (mn * mx == 0.0f) & (numz != 0.0f);
    if (__builtin_amdgcn_ballot_w64(tie)) {
        if (tie) n = crossing(a, b, c, ea, eb, ec);
    }
    return n;
}

// careful form of the crossing test for lanes with an edge function that is exactly zero (the ray passes through an
// edge or a corner: tie rules) -- which includes every triangle that has the query itself as a corner
template <bool kSkipIncident>
__device__ __forceinline__ int crossing_with_ties(const P3 a, const P3 b, const P3 c, float ea, float eb, float ec)
{
    if (kSkipIncident) {
        // faces around the query vertex: the reference's atan2(0,0) = 0 terms; the closing fan stands in for them
        const bool za = (a.x == 0.0f) & (a.y == 0.0f) & (a.z == 0.0f);
        const bool zb = (b.x == 0.0f) & (b.y == 0.0f) & (b.z == 0.0f);
        const bool zc = (c.x == 0.0f) & (c.y == 0.0f) & (c.z == 0.0f);
        if (za | zb | zc) return 0;
    }
    return crossing(a, b, c, ea, eb, ec);
}

// a strip vertex relative to the query, (x, y) as a register pair: the two products of an edge function are ONE packed
// multiplication with crossed halves (v_pk_mul_f32 rounds each product like v_mul_f32: the same bits, still exactly
// antisymmetric), and the subtraction of the query is one packed add
struct S3 { v2f xy; float z; };
__device__ __forceinline__ float edge_fn(const S3& p, const S3& q)
{
    v2f r;                                                        // (p.x q.y, p.y q.x)
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(p.xy), "v"(q.xy));
    float d;                                                      // (in assembly: left to the vectoriser, the difference is
    asm("v_sub_f32 %0, %1, %2" : "=v"(d) : "v"(r.x), "v"(r.y));    // paired with the z subtraction behind three v_mov)
    return d;
}
__device__ __forceinline__ P3 p3(const S3& a) { return P3{a.xy.x, a.xy.y, a.z}; }

// ---- the walk of one leaf strip: box filter for every (ray, element), exact test for the candidates ------------------------
// A wavefront holds up to 64 rays (one per lane) and steps through the strip run [off, off + len), len % 3 == 0.  Of the
// ~145 (ray, element) pairs a ray meets in the leaves it passes, ~10 have the ray's origin inside the projected triangle's
// bounding box at all -- per LANE: almost every element is hit by some lane of the wavefront, so a "does any lane hit"
// branch around the exact test saves nothing.  Hence two stages:
//   filter : the elements' boxes (ray_elem_box, written where the strips are posed) are staged in LDS, see ray_run; four
//            compares per lane set one bit of the lane's mask; after 30 elements the lanes append their candidates
//            (element, lane) to the wavefront's queue in LDS;
//   exact  : whenever the queue holds 64 entries, and at the end of the tile, every lane takes ONE entry: it fetches the
//            entry's ray (ds_bpermute) and the stream elements p-2, p-1, p (from the chunk's copy in LDS), forms the
//            relative coordinates and the SAME three edge functions, determinant, min/max classification and tie path the
//            walk always used; non-zero crossings are added to the ray's counter in LDS, which the ray's own lane
//            flushes once per tile.
// The edge shared with the previous triangle is recomputed from the same floats instead of carried: the same bits.
// Integer sums in any order: the result does not depend on the order of the queue.
//
// Two ray sets per pass.  A leaf's last full tile carries the leaf's remainder as well (RayTile, ray_tile_at): lane l
// holds ray A, pairs[first + l], and for l < n - 64 also ray B, pairs[first + 64 + l].  What a pass pays whatever number
// of its lanes hold a ray -- the record's fetch chain, the staging of each chunk, the flush -- the remainder no longer
// pays a second time; its filter steps it still pays: the staged chunk is filtered once with A's origins and once more
// with B's (ray_run), both sets append to the ONE queue, the exact test takes an entry's ray from set A (ds_bpermute
// from the lane's registers) or set B (org_b in LDS), and the two sets have counters of their own (128 slots).
//
// Bounds: the ring has kRingSize = 128 entries and is indexed modulo 128.  The argument is per TRIP of ray_append, and a
// trip belongs to one set: before a trip the ring holds at most 63 entries (a round of 64 is taken out as soon as it
// holds 64, after every trip, whichever set the trip was for), a trip adds at most 64 (every lane, one entry): at most
// 127.  So no round has to be forced between the two sets' appends, and the ring need not grow for the second set.
// Entries are read back through `& 127` (set << 6 | lane: the counters' 128 slots; `& 63` of it the lane, org_b's 64
// slots) and a clamp to [0, kBoxChunk + 1] (position in the chunk's 64 elements).
// LDS: 512 B ring + 512 B crossings + 1 KB segment counters + 1 KB boxes + 1 KB elements + 1 KB set B's origins = 5 KB
// per wavefront: 32 wavefronts still fit a CU's 160 KB.
//
// WHY THE FILTER NEVER DROPS A PAIR THE FLOAT TEST COUNTS (ties included).  (The argument is about one (ray, element)
// pair: it does not ask which set of which pass the ray rides in.)  Take a pair the filter rejects, say by
// q'x < box.x (the other three sides are mirror images).  The box is decisive (not full), so all corners and the origin
// have |x'|, |y'| <= kBoxRange, and box.x = fl(xmin - kBoxPad) < xmin (kBoxPad >> ulp(kBoxRange)).
//  (1) Relative coordinates are rounded differences: s.x = fl(v'x - q'x) with v'x - q'x > kBoxPad / 2 for all three
//      corners, and rounding is monotone: all three s.x > 0 (no reliance on denormals: the pad keeps them normal).
//      So the three relative corners a, b, c lie in the open half plane x > 0; let theta in (-pi/2, pi/2) be their
//      polar angles as seen from the origin, and |s| <= 2 sqrt 2 kBoxRange =: D.
//  (2) An edge function is e(P,Q) = fl(fl(Px Qy) - fl(Py Qx)).  Rounding is monotone and a difference of two distinct
//      floats is not zero, so e > 0 implies Px Qy > Py Qx exactly, i.e. theta(Q) > theta(P).  If e == 0 the two products
//      rounded to the same float: |Px Qy - Py Qx| <= 2^-24 (|Px Qy| + |Py Qx|) + 2^-148 <= (2^-23 + 2^-100) |P| |Q|
//      (|P| |Q| >= Px Qx >= 2^-28), i.e. |sin(theta(Q) - theta(P))| <= 2^-23 (1 + 2^-70): rounding can turn a strictly
//      negative edge function into 0, never into a positive one.  Either way
//          left_of(e(P,Q), P, Q)  implies  theta(Q) >= theta(P) - eps,   sin eps <= 2^-23 (1 + 2^-70),
//      whatever the lexicographic tie rule answers.
//      In the same way  !left_of(e(P,Q), P, Q)  implies  theta(Q) <= theta(P) + eps.
//  (3) The test counts +-1 only if left_of holds for all of b -> c, c -> a, a -> b, or fails for all of them.  By (2)
//      the three angles then lie within 2 eps of each other: the relative triangle lies in a wedge of
//      half-angle eps at the origin, within D sin eps of its bisector, so its width across the bisector, and with it its
//      smallest altitude, is at most 2 D 2^-23 (1 + 2^-70) < 2^-16.4.
//  (4) The relative corners differ from (corner - origin) by at most 2^-24 * 2 kBoxRange = 2^-19 per coordinate, which
//      changes a width by at most 2 sqrt 2 * 2^-19 = 2^-17.5; ray_elem_box computes the altitude of the stream's floats
//      with an error below 2^-16 (its 2 area is off by at most 8 * 2^-24 times the product of two edges, each at most
//      2 kBoxRange; divided by the longest edge).  So ray_elem_box sees an altitude below
//      2^-16.4 + 2^-17.5 + 2^-16 < 2^-14.9 < kBoxSliver = 2^-14 -- and gave that element the FULL box, which rejects
//      nothing.  Contradiction: a rejected pair counts 0 in the float test.
// Slivers in projection (triangles nearly parallel to the ray, whose line passes through the origin while the origin lies
// beyond their end, two edge functions rounding to zero) are exactly the case of (3); corners or origins beyond kBoxRange,
// NaN included, never reach a decisive compare: such an element has the full box, such a lane compares NaN (passes all).
// The comparisons are inclusive and written as negations so that NaN passes; pad, range and sliver bound are parts of
// this argument, not tuning knobs.
constexpr int kRingSize = 128;
constexpr int kPassRays = 2 * kRayQueries;     // rays of one pass: set A and set B
struct RayQueue {
    uint32_t ring[kRingSize];                  // (element's position in the chunk << 7) | ray of the pass (set << 6 | lane)
    int32_t cross[kPassRays];                  // crossings of the pass's rays
    uint32_t seg[2][kPassRays];                // kSeg: per-segment crossings, four byte counters per word (see below)
    float4 box[64];                            // the boxes of the kBoxChunk elements being filtered (+ 3 readable behind them)
    RayElem elem[64];                          // ... and the elements themselves, from two before the chunk
    float4 org_b[kRayQueries];                 // set B's rays: sheared origin (x', y', z) and, as bits, the segments word
};
constexpr int kBoxChunk = 60;
// What a lane knows about the pass: its own ray of set A in registers (the exact test fetches an entry's ray from its
// lane, ds_bpermute); whether the pass has a set B (two: wave-uniform) and whether the lane holds one of its rays.  Set B's
// rays live in LDS (RayQueue::org_b): in registers beside A's they cost the kernel two wavefronts per SIMD.
struct RayLane { float qx, qy, qz; int qmask; bool active, two, active_b; };
// the origin the filter compares: beyond the range the boxes decide for (or NaN) it is compared as NaN and passes every box
__device__ __forceinline__ float ray_filter_origin(float v, float qx, float qy)
{
    return ((__builtin_fabsf(qx) <= kBoxRange) & (__builtin_fabsf(qy) <= kBoxRange)) ? v : __builtin_nanf("");
}

// kSeg: the element's word holds the segments that list its triangle as a face (bits 24-31), qmask the segments the
// ray's query vertex belongs to: the crossing also goes into per-segment counts (the segment test of winding.hip needs,
// for every segment vertex, its crossings with the faces of its own segments only).  Eight counters as bytes of two
// words: bits 0-3 of (em & qmask) are spread to the byte positions by one multiplication; a running word may borrow
// across its bytes, the final word is the exact sum all the same (seg_leaf_count).
template <bool kSkipIncident, bool kSeg>
__device__ __forceinline__ void ray_exact(RayQueue& q, uint32_t& head, int n, const RayLane& me, int lane)
{
    __syncthreads();                                              // (one wavefront per workgroup) the appends are visible
    const bool valid = lane < n;
    const uint32_t ent = q.ring[(head + (uint32_t)lane) & (kRingSize - 1)];
    head += (uint32_t)n;
    const int r = (int)(ent & (uint32_t)(kPassRays - 1));         // the counters' index: set << 6 | lane
    const uint32_t k = min(ent >> 7, (uint32_t)(kBoxChunk + 1));       // elem[k + 2] is the element, elem[k], elem[k + 1] its predecessors
    // the entry's ray: every lane is active here (a bpermute from an inactive lane reads 0)
    const int rl = (r & (kRayQueries - 1)) << 2;
    float ox = __int_as_float(__builtin_amdgcn_ds_bpermute(rl, __float_as_int(me.qx)));
    float oy = __int_as_float(__builtin_amdgcn_ds_bpermute(rl, __float_as_int(me.qy)));
    float oz = __int_as_float(__builtin_amdgcn_ds_bpermute(rl, __float_as_int(me.qz)));
    int om = kSeg ? __builtin_amdgcn_ds_bpermute(rl, me.qmask) : 0;
    if (me.two) {                      // wave-uniform: an entry of set B takes its ray from LDS instead, one read and four selects
        const bool from_b = r >= kRayQueries;
        const float4 ob = q.org_b[r & (kRayQueries - 1)];
        ox = from_b ? ob.x : ox; oy = from_b ? ob.y : oy; oz = from_b ? ob.z : oz;
        if (kSeg) om = from_b ? __float_as_int(ob.w) : om;
    }
    const RayElem el0 = q.elem[k], el1 = q.elem[k + 1], el2 = q.elem[k + 2];
    const v2f oxy = {ox, oy};
    S3 s0, s1, s2;
    s0.xy = (v2f){el0.x, el0.y} - oxy; s0.z = el0.z - oz;
    s1.xy = (v2f){el1.x, el1.y} - oxy; s1.z = el1.z - oz;
    s2.xy = (v2f){el2.x, el2.y} - oxy; s2.z = el2.z - oz;
    // edge function of the edge opposite each corner, in stream order p-2 -> p-1 -> p
    const float e0 = edge_fn(s1, s2), e1 = edge_fn(s2, s0), e2 = edge_fn(s0, s1);
    // triangle (p-2, p-1, p): det = sum of (edge function opposite a corner) x (that corner's depth)
    const float numz = __builtin_fmaf(e2, s2.z, __builtin_fmaf(e1, s1.z, e0 * s0.z));
    const float mn = __builtin_fminf(__builtin_fminf(e0, e1), e2);
    const float mx = __builtin_fmaxf(__builtin_fmaxf(e0, e1), e2);
    // generic position: the origin is inside the projection iff the edge functions have one sign, the hit is in
    // front iff det has that sign too; +1 (leaving through the front) for the positive orientation, -1 for the
    // negative one.  The faces around a query vertex (two edge functions through the origin, det exactly 0)
    // count 0 here, as they must.
    int c = (int)(__builtin_fminf(mn, numz) > 0.0f) - (int)(__builtin_fmaxf(mx, numz) < 0.0f);
    // exact ties: some edge function is zero (mn * mx == 0: all are >= 0 or all <= 0 then) and det is not, i.e. the
    // ray passes through an edge or a corner of a triangle that does not contain the query
    const bool tie = (mn * mx == 0.0f) & (numz != 0.0f);
    if (__builtin_amdgcn_ballot_w64(tie)) {
        if (tie) c = crossing_with_ties<kSkipIncident>(p3(s0), p3(s1), p3(s2), e0, e1, e2);
    }
    // the element's fourth word: orientation (integer, bits 0-23; 0 for a priming element, which then adds nothing) and
    // segments (bits 24-31), see RayElem
    const int word = __float_as_int(el2.sign);
    const int cs = c * ((word << 8) >> 8);
    if (valid && cs != 0) {
        atomicAdd(&q.cross[r], cs);
        if (kSeg) {
            const uint32_t t = ((uint32_t)word >> 24) & (uint32_t)om;
            if (t & 15u) atomicAdd(&q.seg[0][r], (uint32_t)cs * (((t & 15u) * 0x00204081u) & 0x01010101u));
            if (t >> 4) atomicAdd(&q.seg[1][r], (uint32_t)cs * ((((t >> 4) & 15u) * 0x00204081u) & 0x01010101u));
        }
    }
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The filter of one element: bit K of the lane's mask is set iff the lane's origin lies in the element's box.  Four
// compares that narrow EXEC and one OR under what is left of it: five
// vector instructions, one scalar one (EXEC back to `all`, the wavefront's lanes) and no branch per element.  Inclusive
// and written as negations -- !(lo > f), !(hi < f): NaN passes.
template <int K>
__device__ __forceinline__ void ray_filter(const float4 box, unsigned long long all, float fx, float fy, uint32_t& mask)
{
    asm volatile("v_cmpx_ngt_f32 vcc, %[lox], %[fx]\n\t"
                 "v_cmpx_nlt_f32 vcc, %[hix], %[fx]\n\t"
                 "v_cmpx_ngt_f32 vcc, %[loy], %[fy]\n\t"
                 "v_cmpx_nlt_f32 vcc, %[hiy], %[fy]\n\t"
                 "v_or_b32 %[m], %[bit], %[m]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [m] "+v"(mask)
                 : [lox] "v"(box.x), [hix] "v"(box.y), [loy] "v"(box.z), [hiy] "v"(box.w), [bit] "n"(1u << K), [sv] "s"(all),
                   [fx] "v"(fx), [fy] "v"(fy)
                 : "vcc");
}

// the lanes' candidate bits of the chunk's elements base .. base + 29 go to the queue: per trip every lane that has one left
// appends its lowest (the trips: the largest number of candidates any one ray has in the chunk, ~2.3 on average).
// `ray`: set << 6 | lane, the lane's ray of the set whose verdicts `mask` holds.
template <bool kSkipIncident, bool kSeg>
__device__ __forceinline__ void ray_append(uint32_t mask, int base, RayQueue& q, uint32_t& head, uint32_t& tail,
                                           const RayLane& me, int lane, uint32_t ray)
{
    unsigned long long m;
    while ((m = __builtin_amdgcn_ballot_w64(mask != 0u)) != 0ull) {
        if (mask != 0u) {
            const int k = __builtin_ctz(mask);
            mask &= mask - 1u;
            q.ring[(tail + lanes_below(m)) & (kRingSize - 1)] = ((uint32_t)(base + k) << 7) | ray;
        }
        tail += (uint32_t)__builtin_popcountll(m);
        if (tail - head >= 64u) ray_exact<kSkipIncident, kSeg>(q, head, 64, me, lane);
    }
}

// One leaf strip, elements [off, off+len), len % 3 == 0.  The wavefront was waiting, not computing: with the boxes (before:
// the elements) fetched three at a time one trip ahead, every trip waited for a round trip to the L2.  So the boxes of up
// to kBoxChunk = 60 elements, and the elements from two before them, are fetched by ONE load each, a box and an element
// per lane, and put into LDS (ray_stage): the filter reads the boxes back from there, all lanes the same three per trip and
// one trip ahead, and the exact test its three elements; the filter's verdicts on 30 elements are bits 0-29 of one register
// per lane.  `staged`: the run's first chunk is in LDS already -- a tile's first chunk is fetched with the tile's record
// while the pass before is walked, and staged before the next record is fetched, so that its eight registers are free by then.
__device__ __forceinline__ void ray_stage(RayQueue& q, int lane, const float4 box, const RayElem el)
{
    __syncthreads();                                    // (one wavefront per workgroup) the last chunk has been read
    q.box[lane] = box;
    q.elem[lane] = el;
}

template <bool kSkipIncident, bool kSeg>
__device__ __forceinline__ void ray_run(const RayElem* __restrict__ st, const float4* __restrict__ boxes, int off, int len, int T,
                                        RayQueue& q, uint32_t& head, uint32_t& tail, const RayLane& me, int lane, bool staged)
{
    const unsigned long long all = __builtin_amdgcn_read_exec();     // every lane of the wavefront: the walk is not divergent
    for (int c0 = 0; c0 < len; c0 += kBoxChunk) {
    if (!(staged && c0 == 0)) {
        const float4 mine = boxes[min(off + c0 + lane, T - 1)];
        const RayElem mine_el = st[min(max(off + c0 - 2 + lane, 0), T - 1)];
        // the queue's entries name positions in the chunk that is about to go (only runs of more than kBoxChunk elements
        // and the block-major order get here with entries queued; a pass begins with the queue empty)
        while (tail != head) ray_exact<kSkipIncident, kSeg>(q, head, (int)min(tail - head, 64u), me, lane);
        ray_stage(q, lane, mine, mine_el);
    }
    __syncthreads();
    // The staged chunk is filtered for set A and, in a pass that has one, once more for set B: the same loop with B's
    // origin, chosen here, once per chunk and set (wave-uniform), not per element.  Both sets' candidates name positions
    // in this chunk, so both go to the queue before the next chunk is staged.
#pragma unroll 1
    for (int set = 0; set < (me.two ? 2 : 1); ++set) {
    float ox = me.qx, oy = me.qy;
    bool active = me.active;
    if (set) { const float4 ob = q.org_b[lane]; ox = ob.x; oy = ob.y; active = me.active_b; }
    const float fx = ray_filter_origin(ox, ox, oy), fy = ray_filter_origin(oy, ox, oy);
    const uint32_t ray = (uint32_t)(set * kRayQueries + lane);
    const float4* p = q.box;
    int at = 0, left = min(len - c0, kBoxChunk);
    // three elements: bits 3 J .. 3 J + 2; the next three boxes are read meanwhile.  Unrolled by hand: the bits are
    // literals, the boxes stay where their loads put them, and a 32-bit count is compared on the scalar unit
#define TUCH_RAY_TRIPLE(J, AHEAD)                                                  \
    {                                                                              \
        const float4 b0 = n0, b1 = n1, b2 = n2;                                    \
        if (AHEAD) { n0 = p[3]; n1 = p[4]; n2 = p[5]; }                            \
        ray_filter<3 * J>(b0, all, fx, fy, mask);                                  \
        ray_filter<3 * J + 1>(b1, all, fx, fy, mask);                              \
        ray_filter<3 * J + 2>(b2, all, fx, fy, mask);                              \
        left -= 3; p += 3;                                                         \
        asm("" : "+s"(left));                                                      \
    }
    while (left > 0) {
        // every group of 30 reads its first three boxes itself: carried over from the group before, the boxes read ahead
        // stayed live past every way out of the group, and leaving after triple J (0 .. 9) cost 6 min(J, 8) register moves
        // that put them where a next group would expect them (48 for a run of 30 elements, which has no next group)
        float4 n0 = p[0], n1 = p[1], n2 = p[2];
        uint32_t mask = 0u;
        do {
            TUCH_RAY_TRIPLE(0, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(1, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(2, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(3, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(4, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(5, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(6, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(7, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(8, true) if (left <= 0) break;
            TUCH_RAY_TRIPLE(9, false)
        } while (false);
        if (!active) mask = 0u;                         // a padding lane repeats another lane's ray
        ray_append<kSkipIncident, kSeg>(mask, at, q, head, tail, me, lane, ray);
        at += 30;
    }
    }
    }
#undef TUCH_RAY_TRIPLE
}

// what a pass found for one ray: its crossings and (kSeg) the two words of per-segment byte counters
struct RaySums { int crossings; uint32_t pa, pb; };

// the end of a pass: the rest of the queue, then every lane takes the sums of its own ray of set A -- and of set B where
// the pass has one: the two sets have counters of their own -- and leaves the counters zero
template <bool kSkipIncident, bool kSeg>
__device__ __forceinline__ void ray_flush(RayQueue& q, uint32_t& head, uint32_t tail, const RayLane& me, int lane,
                                          RaySums& a, RaySums& b)
{
    while (tail != head) ray_exact<kSkipIncident, kSeg>(q, head, (int)min(tail - head, 64u), me, lane);
    __syncthreads();
    a.crossings = q.cross[lane];
    q.cross[lane] = 0;
    if (kSeg) {
        a.pa = q.seg[0][lane]; a.pb = q.seg[1][lane];
        q.seg[0][lane] = 0u; q.seg[1][lane] = 0u;
    }
    if (me.two) {
        b.crossings = q.cross[kRayQueries + lane];
        q.cross[kRayQueries + lane] = 0;
        if (kSeg) {
            b.pa = q.seg[0][kRayQueries + lane]; b.pb = q.seg[1][kRayQueries + lane];
            q.seg[0][kRayQueries + lane] = 0u; q.seg[1][kRayQueries + lane] = 0u;
        }
    }
}

// ---- which leaves can the rays of a 64-query block meet? -------------------------------------------------------------
// A ray can only cross faces of a leaf whose 9-slab volume it meets.  Slabs whose functional does not change along
// the ray (x, y, x+y, x-y in the sheared frame) bound the query from both sides, those that grow along it (z, x+z,
// y+z) only from above, those that shrink (x-z, y-z) only from below.  One wavefront per (block, body):
//   stage 1, lanes over LEAVES: the ranges of the block's 64 queries against every leaf's slabs (a superset);
//   stage 2, lanes over QUERIES: the surviving leaves tested query by query (wave-uniform leaf, scalar loads).
// Output: the strip ranges (ex_off, ex_len) of the leaves some ray of the block can meet, and how many.  No tree
// descent: with ~215 leaves the flat test is four rounds of 64 lanes, and nothing in it waits on a parent's verdict.
constexpr int kFallbackChunks = 8;            // wavefronts per query block when a body falls back to block-major order

__device__ __forceinline__ int wave_min_i32(int v)                                      // as common.h's wave_max_uniform_i32
{
    TUCH_WAVE_REDUCE("v_min_i32_dpp");
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_max_i32(int v) { return wave_max_uniform_i32(v); }
// v_writelane_b32: `old` with lane `lane` (wave-uniform) replaced by the wave-uniform `value`.  Declared by the intrinsic's own
// name (clang has no builtin for it), so that the compiler sees it and keeps the wait states behind a compare
extern "C" __device__ int tuch_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// One (query block, leaf) the block has to visit: which of its 64 rays pass the leaf's slabs.
// (RayEntry, RayTile, RayBody: model.h)

// ---- the 13-slab test on packed 16-bit levels -------------------------------------------------------------------------------
// record (ray_leaf_bounds_kernel): s0 = (lo0,lo1) (lo3,lo4) (lo6,lo8) (hi0,hi1)   s1 = (hi2,hi3) (hi4,hi5) (hi7,leaf) node
// with the slabs 0..8 = x y z x+y x-y x+z x-z y+z y-z.  A ray (or a block's range) is the seven dwords that pair up with
// them: u* hold the values set against LOWER bounds, rounded UP (the block: their maxima), d* those set against UPPER
// bounds, rounded DOWN (the block: their minima); the upper half of d3 faces the record's leaf number and holds kNearMin.
struct NearSide { uint32_t u0, u1, u2, d0, d1, d2, d3; };
typedef short near_s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_sub_sat(uint32_t a, uint32_t b)      // v_pk_sub_i16 ... clamp: a - b per half, saturating
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(near_s16x2, a), __builtin_bit_cast(near_s16x2, b)));
}
// Outside some slab: lo > u or d > hi for one of the 13 pairs, i.e. one of the saturating differences u - lo, hi - d is
// NEGATIVE (a saturating difference has the sign of the exact one; 0 passes).  Seven packed subtractions, the sign bits
// gathered by three 3-input ORs and one AND: 12 vector instructions with the compare, where 13 single-precision
// differences (v_fma_mix_f32) under six v_max3_f32 were 20.  leaf - kNearMin >= 0 for every 16-bit leaf: the 14th half
// never rejects.  One routine for both stages: stage 1 passes the block's ranges as `r` (wave-uniform) with 64 records in
// the lanes, stage 2 the lanes' rays with one record.
__device__ __forceinline__ bool near_outside(const uint4& s0, const uint4& s1, const NearSide& r)
{
    const uint32_t neg = pk_sub_sat(r.u0, s0.x) | pk_sub_sat(r.u1, s0.y) | pk_sub_sat(r.u2, s0.z) | pk_sub_sat(s0.w, r.d0) |
                         pk_sub_sat(s1.x, r.d1) | pk_sub_sat(s1.y, r.d2) | pk_sub_sat(s1.z, r.d3);
    return (neg & 0x80008000u) != 0u;
}
// One unit of work of ray_leaf_kernel: up to 64 rays (pairs[first .. first + n)) against one leaf's strip run.
// per body: number of tiles, whether the pair list overflowed (the body is then walked block-major)

// One workgroup of kWaves wavefronts per (block of 64 queries, body); every wavefront holds the block's 64 queries.
//   ranges : the 13 block ranges (kWaves = 4: each reduced by one of the wavefronts, shared through LDS);
//   rounds : the wavefronts take one chunk of 64 leaves each, lanes over LEAVES: block ranges against the slabs
//            (stage 1); the records of the passing leaves go to a queue in LDS; the queue is then dealt out evenly,
//            two entries per wavefront and trip: every ray against the record (stage 2).
// A trip of stage 2 is a dependent chain (LDS read -> test -> compare -> hand-over; ~450 clocks measured with the cycle
// counter when the test was 19 single-precision instructions) and the blocks through the trunk pass five times the
// average number of leaves: the time of the kernel is that of its slowest workgroup plus the rounds of workgroups the chip
// needs -- at batch 64, with 6.75 wavefronts resident per SIMD, the vector instructions of its heaviest SIMDs.  With one
// wavefront testing a block's leaves one at a time it was 59 us at batch 64 and 41 us at batch 8.  Four wavefronts and
// two chains per trip: 16 us at batch 8 (10 us with the packed test).  At batch 64 the search runs beside this kernel on another stream and leaves 7 wave slots and < 4 KB of
// LDS per CU (v2v.hip, leave_room): there the one-wavefront form (2 KB) is used -- workgroups of four with an 8 KB
// queue waited for LDS until the search had drained (202 us, tools/graph_timeline.py).
//
// THE NUMBERS.  Records and rays are near_encode levels (16-bit fixed point, one scale).  ray_leaf_bounds_kernel forms the
// padded single-precision bounds lo, hi of a leaf relative to the body's reference point -- the numbers the test trusted
// when it compared in single precision -- and stores floor(lo S), ceil(hi S); this kernel forms the rays' nine values r in
// single precision as it always did and converts each ONCE per wavefront: ceil(r S) where it meets a lower bound,
// floor(r S) where it meets an upper bound, every conversion saturating to the code that cannot reject.
// NO PAIR IS DROPPED: a rejection is lo_fx > up(r) (or dn(r) > hi_fx, its mirror image).  A lo_fx that saturated to kNearMin
// exceeds nothing and an up(r) that saturated to kNearMax is exceeded by nothing; in every other case lo_fx <= lo S and
// up(r) >= r S (a clamp from the far side moves a level the same way as its rounding).  So lo_fx > up(r) implies
// lo S > r S, lo > r: the single-precision
// bound, whose pads cover the roundings of the projections and are unchanged, rejects as well.  Directed, monotone,
// saturating conversion can only turn a rejection into a pass.  The lists are a superset of the pairs that can cross; the
// walk filters every (ray, element) by its box and then tests exactly (ray_exact), so an extra pair costs lanes, never a
// count: crossing counts and flags are what they were, bit for bit.
// STAGE 1 IS A SUPERSET OF STAGE 2: the block's side holds, half by half, the maximum of the lanes' u-levels and the
// minimum of their d-levels (padding lanes repeat a real query), both stages run near_outside on the same record, and a
// saturating difference is monotone in either operand: u_block - lo >= u_ray - lo and hi - d_block >= hi - d_ray.  A
// negative difference in stage 1 is therefore negative for every ray; a leaf that some ray passes in stage 2 passed stage 1.
// ENTRIES ARE WRITTEN BY LANES: a stage-2 trip leaves its hit masks (wave-uniform) in the lanes that own the trip's queue
// positions (v_writelane); after the round's trips every owner of a non-empty mask takes the next slot in queue order and
// writes its entry and its leaf's ray count: one store and one atomic INSTRUCTION per round, where every hit had its own
// single-lane region.  Queue order is leaf order, so a one-wavefront block's list ascends in the leaf number.
template <bool kVerts, int kWaves>
__global__ __launch_bounds__(64 * kWaves) void ray_near_kernel(
    const float* __restrict__ pts, const TreeNode* __restrict__ nodes, const float* __restrict__ bounds, int N,
    int num_leaves, const int32_t* __restrict__ qperm,
    const int32_t* __restrict__ counts, int Q, int qblocks, RayEntry* __restrict__ lists, int32_t* __restrict__ list_len,
    int32_t* __restrict__ leaf_cnt,             // [B][num_leaves], zeroed: rays per leaf
    unsigned long long* __restrict__ stats,     // measurement (or nullptr): [1] += (ray, element) pairs inside a listed
                                                // leaf's slabs, [2] += 64 x elements listed
    float* __restrict__ rays_out)               // tuch_ray_near_debug (or nullptr): [B][qblocks * 64][9], the rays' values
{
    __builtin_amdgcn_s_setprio(3);               // (see ray_tiles_fill_kernel)
    const int qb = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
    const int wave = kWaves > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    __shared__ uint4 queue[64 * kWaves][2];     // records of the round's leaves that passed stage 1
    __shared__ int range[16];
    __shared__ int queued[2], slots;            // queue entries (rounds in turn); list entries written (slots are taken from it)
    int i0;
    bool real;                                  // padding lanes repeat a query; they are left out of the masks
    if (kVerts) {
        i0 = qperm[qb * kRayQueries + lane];
        real = qb * kRayQueries + lane < Q;
    } else {
        const int n = counts ? counts[b] : Q;
        if (qb * kRayQueries >= n) {
            if (threadIdx.x == 0) list_len[(size_t)b * qblocks + qb] = 0;
            return;
        }
        i0 = min(qb * kRayQueries + lane, n - 1);
        real = qb * kRayQueries + lane < n;
    }
    if (threadIdx.x == 0) { queued[0] = 0; queued[1] = 0; slots = 0; }
    const unsigned long long real_mask = __builtin_amdgcn_ballot_w64(real);
    // every load that does not wait for the block's ranges is issued here: the body's reference point and the
    // records of the wavefront's first chunk of leaves
    const float4 ctr = *reinterpret_cast<const float4*>(bounds + near_centres_at(gridDim.y, num_leaves) + (size_t)b * 4);
    const uint4* recs = reinterpret_cast<const uint4*>(bounds + near_records_at(gridDim.y, num_leaves)) + (size_t)b * num_leaves * 2;
    // stage 1 reads the leaves' 32-byte RECORDS only (what stage 2 tests every ray against) -- with 13 single-precision
    // slab values beside them every block fetched 84 bytes per leaf, 257 MB per launch at batch 64 out of the L2s: the
    // kernel's time then.
    struct Chunk { uint4 r0, r1; };
    auto load_chunk = [&](int base) {
        Chunk c;
        const int lc = min(base + lane, num_leaves - 1);
        c.r0 = recs[lc * 2];
        c.r1 = recs[lc * 2 + 1];
        return c;
    };
    Chunk nxt = load_chunk(wave * 64);
    const float* q3 = pts + ((size_t)b * Q + i0) * 3;
    const float qz = q3[2];
    const float qx = shear_x(q3[0], qz), qy = shear_y(q3[1], qz);
    // the queries relative to the body's reference point, as the records are
    const float rx = qx - ctr.x, ry = qy - ctr.y, rz = qz - ctr.z;
    const float r4 = rx + ry, r5 = rx - ry, r6 = rx + rz, r7 = rx - rz, r8 = ry + rz, r9 = ry - rz;
    if (rays_out && wave == 0) {
        float* o = rays_out + (((size_t)b * qblocks + qb) * kRayQueries + lane) * 9;
        o[0] = rx; o[1] = ry; o[2] = rz; o[3] = r4; o[4] = r5; o[5] = r6; o[6] = r7; o[7] = r8; o[8] = r9;
    }
    // ... as levels, once per wavefront: up against the lower bounds, down against the upper bounds
    const int ux = near_encode(rx, true), uy = near_encode(ry, true), u4 = near_encode(r4, true), u5 = near_encode(r5, true);
    const int u7 = near_encode(r7, true), u9 = near_encode(r9, true);
    const int dx = near_encode(rx, false), dy = near_encode(ry, false), dz = near_encode(rz, false), d4 = near_encode(r4, false);
    const int d5 = near_encode(r5, false), d6 = near_encode(r6, false), d8 = near_encode(r8, false);
    const NearSide me = {near_pack(ux, uy), near_pack(u4, u5), near_pack(u7, u9), near_pack(dx, dy),
                         near_pack(dz, d4), near_pack(d5, d6), near_pack(d8, kNearMin)};
    // the block's side: the largest u and the smallest d of its lanes (integers: a NaN query is a saturated level here)
    NearSide blk;
    if (kWaves == 4) {
        if (wave == 0) {
            const int a = wave_max_i32(ux), c = wave_max_i32(uy), d = wave_min_i32(dx), e = wave_min_i32(dy);
            if (lane == 0) { range[0] = a; range[1] = c; range[2] = d; range[3] = e; }
        } else if (wave == 1) {
            const int a = wave_max_i32(u4), c = wave_max_i32(u5), d = wave_min_i32(d4), e = wave_min_i32(d5);
            if (lane == 0) { range[4] = a; range[5] = c; range[6] = d; range[7] = e; }
        } else if (wave == 2) {
            const int a = wave_min_i32(dz), c = wave_min_i32(d6), d = wave_max_i32(u7);
            if (lane == 0) { range[8] = a; range[9] = c; range[10] = d; }
        } else {
            const int a = wave_min_i32(d8), c = wave_max_i32(u9);
            if (lane == 0) { range[11] = a; range[12] = c; }
        }
        __syncthreads();
        auto at = [&](int k) { return __builtin_amdgcn_readfirstlane(range[k]); };
        blk = NearSide{near_pack(at(0), at(1)), near_pack(at(4), at(5)), near_pack(at(10), at(12)), near_pack(at(2), at(3)),
                       near_pack(at(8), at(6)), near_pack(at(7), at(9)), near_pack(at(11), kNearMin)};
    } else {
        blk = NearSide{near_pack(wave_max_i32(ux), wave_max_i32(uy)), near_pack(wave_max_i32(u4), wave_max_i32(u5)),
                       near_pack(wave_max_i32(u7), wave_max_i32(u9)), near_pack(wave_min_i32(dx), wave_min_i32(dy)),
                       near_pack(wave_min_i32(dz), wave_min_i32(d4)), near_pack(wave_min_i32(d5), wave_min_i32(d6)),
                       near_pack(wave_min_i32(d8), kNearMin)};
    }
    RayEntry* list = lists + ((size_t)b * qblocks + qb) * num_leaves;
    unsigned long long useful = 0, listed = 0;  // (per lane: summed by the atomics at the end)
    int nslots = 0;                             // one wavefront: the list's length in a (scalar) register, no LDS atomic
    // the hit mask of one queue position, handed to the lane that owns the position
    uint32_t own_lo = 0u, own_hi = 0u;
    auto hand = [&](unsigned long long hit, int owner) {
        own_lo = (uint32_t)tuch_writelane((int)(uint32_t)hit, owner, (int)own_lo);
        own_hi = (uint32_t)tuch_writelane((int)(uint32_t)(hit >> 32), owner, (int)own_hi);
    };
    // (one wavefront: its LDS accesses are served in order, nothing to wait for between the stages)
    auto sync = [&] { if (kWaves > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier(); };
    for (int round = 0; round * 64 * kWaves < num_leaves; ++round) {
        const int base = (round * kWaves + wave) * 64;
        const Chunk c = nxt;
        if (base + 64 * kWaves < num_leaves) nxt = load_chunk(base + 64 * kWaves);
        // (the two conditions meet as masks: a ballot of their conjunction is rebuilt from a 0 / 1 register)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(!near_outside(c.r0, c.r1, blk)) &
                                        __builtin_amdgcn_ballot_w64(base + lane < num_leaves);
        const bool pass = (mask >> lane) & 1ull;
        if (mask) {
            int at = 0;
            if (kWaves > 1) {
                if (lane == 0) at = atomicAdd(&queued[round & 1], __builtin_popcountll(mask));
                at = __builtin_amdgcn_readfirstlane(at);
            }
            at += __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
            if (pass) { queue[at][0] = c.r0; queue[at][1] = c.r1; }
        }
        sync();
        const int n = kWaves > 1 ? __builtin_amdgcn_readfirstlane(queued[round & 1]) : __builtin_popcountll(mask);
        if (kWaves > 1 && threadIdx.x == 0) queued[(round + 1) & 1] = 0;    // (last read before this round's first barrier)
        own_lo = 0u; own_hi = 0u;
        int pos;                                // the queue position this lane owns in this round
        if (kWaves == 1) {
            // one wavefront per block (large batches): FOUR records per trip -- the trip is a dependent chain (LDS read ->
            // 12 vector instructions -> compare -> two v_writelane) and the blocks through the trunk have ~200 records
            pos = lane;
            for (int i = 0; i < n; i += 4) {
                // (i + 3 <= 63: n <= 64, i % 4 == 0.  Positions behind the queue's end hold whatever LDS held: their masks go
                // to owners >= n, which write nothing)
                const uint4 a0 = queue[i][0], a1 = queue[i][1], c0 = queue[i + 1][0], c1 = queue[i + 1][1];
                const uint4 d0 = queue[i + 2][0], d1 = queue[i + 2][1], f0 = queue[i + 3][0], f1 = queue[i + 3][1];
                const bool out_a = near_outside(a0, a1, me), out_c = near_outside(c0, c1, me);
                const bool out_d = near_outside(d0, d1, me), out_f = near_outside(f0, f1, me);
                hand(__builtin_amdgcn_ballot_w64(!out_a) & real_mask, i);
                hand(__builtin_amdgcn_ballot_w64(!out_c) & real_mask, i + 1);
                hand(__builtin_amdgcn_ballot_w64(!out_d) & real_mask, i + 2);
                hand(__builtin_amdgcn_ballot_w64(!out_f) & real_mask, i + 3);
            }
        } else {
            // trip t of wavefront w tests the positions w * 2 + t * 8 + {0, 1}; lanes 2 t, 2 t + 1 own them (t < 32: the queue
            // holds at most 64 kWaves records)
            pos = wave * 2 + (lane >> 1) * (kWaves * 2) + (lane & 1);
            int owner = 0;
            for (int i = wave * 2; i < n; i += kWaves * 2, owner += 2) {
                const uint4 a0 = queue[i][0], a1 = queue[i][1], c0 = queue[i + 1][0], c1 = queue[i + 1][1];   // (i + 1 <= 255)
                const bool out_a = near_outside(a0, a1, me), out_c = near_outside(c0, c1, me);
                hand(__builtin_amdgcn_ballot_w64(!out_a) & real_mask, owner);
                hand(__builtin_amdgcn_ballot_w64(!out_c) & real_mask, owner + 1);       // (i + 1 == n: its owner writes nothing)
            }
        }
        // the owners of non-empty masks write the entries
        const bool has = pos < n && (own_lo | own_hi) != 0u;
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(has);
        if (hm) {
            int at = nslots;
            if (kWaves == 1) {
                nslots += __builtin_popcountll(hm);
            } else {
                if (lane == 0) at = atomicAdd(&slots, __builtin_popcountll(hm));
                at = __builtin_amdgcn_readfirstlane(at);
            }
            if (has) {
                const uint4 who = queue[pos][1];
                const int leaf = (int)(who.z >> 16), nd = (int)who.w;
                const int rays = __builtin_popcount(own_lo) + __builtin_popcount(own_hi);
                const int slot = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0));
                list[slot] = RayEntry{leaf, nd, own_lo, own_hi};
                atomicAdd(&leaf_cnt[(size_t)b * num_leaves + leaf], rays);
                if (stats) {
                    const int len = nodes[nd].ex_len;
                    useful += (unsigned long long)rays * len;
                    listed += 64ull * len;
                }
            }
        }
        sync();
    }
    if (stats && listed) { atomicAdd(stats + 1, useful); atomicAdd(stats + 2, listed); }
    if (threadIdx.x == 0) list_len[(size_t)b * qblocks + qb] = kWaves == 1 ? nslots : slots;
}

// Per body: where every leaf's rays start in the pair list (exclusive scan of the counts) and the table of tiles
// (leaf, 64 of its rays; the leaf's last tile takes the c % 64 left over as well, see RayTile: a tile costs the walk the
// same fetch chain, staging and flush whether it holds 3 rays or 64, and 64 + c % 64 rays are still one pass).  A body
// whose pairs do not fit `cap` is marked: it is walked block-major instead.
__device__ __forceinline__ int ray_tile_count(int c) { return c >= 64 ? c >> 6 : (c > 0 ? 1 : 0); }
// tile k of a leaf with c rays whose range in the pair list starts at `off`
__device__ __forceinline__ RayTile ray_tile_at(int ex_off, int ex_len, int off, int c, int k)
{
    return RayTile{ex_off, ex_len, off + 64 * k, k + 1 == ray_tile_count(c) ? c - 64 * k : 64};
}
constexpr int kTilesBlock = 256;
__global__ __launch_bounds__(kTilesBlock) void ray_tiles_kernel(
    const int32_t* __restrict__ leaf_cnt, const TreeNode* __restrict__ nodes, const int32_t* __restrict__ leaf_nodes,
    int num_leaves, int cap, int max_tiles, int fallback_tiles, int32_t* __restrict__ leaf_off,
    RayTile* __restrict__ tiles, RayBody* __restrict__ body)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const int per = (num_leaves + kTilesBlock - 1) / kTilesBlock;
    const int l0 = min(t * per, num_leaves), l1 = min(l0 + per, num_leaves);
    const int32_t* cnt = leaf_cnt + (size_t)b * num_leaves;
    int pairs = 0, ntile = 0;
    for (int l = l0; l < l1; ++l) { pairs += cnt[l]; ntile += ray_tile_count(cnt[l]); }
    __shared__ int sp[kTilesBlock], st[kTilesBlock];
    sp[t] = pairs;
    st[t] = ntile;
    __syncthreads();
    for (int d = 1; d < kTilesBlock; d <<= 1) {          // inclusive scans
        const int ap = t >= d ? sp[t - d] : 0, at = t >= d ? st[t - d] : 0;
        __syncthreads();
        sp[t] += ap;
        st[t] += at;
        __syncthreads();
    }
    const int total_pairs = sp[kTilesBlock - 1], total_tiles = st[kTilesBlock - 1];
    const bool overflow = total_pairs > cap || total_tiles > max_tiles;
    if (t == 0) body[b] = RayBody{overflow ? fallback_tiles : total_tiles, overflow ? 1 : 0};
    if (overflow) return;
    int off = sp[t] - pairs, tile = st[t] - ntile;
    RayTile* out = tiles + (size_t)b * max_tiles;
    for (int l = l0; l < l1; ++l) {
        leaf_off[(size_t)b * num_leaves + l] = off;
        const TreeNode nd = nodes[leaf_nodes[l]];
        for (int k = 0; k < ray_tile_count(cnt[l]); ++k) out[tile++] = ray_tile_at(nd.ex_off, nd.ex_len, off, cnt[l], k);
        off += cnt[l];
    }
}

// The rays of every leaf: slot (= position of the query in its body's order) of each set bit of every entry.
// The order within a leaf's range comes from an atomic counter and may vary between runs; the crossing counts
// are integer sums and do not depend on it.
__global__ __launch_bounds__(64) void ray_fill_kernel(
    const RayEntry* __restrict__ lists, const int32_t* __restrict__ list_len, const RayBody* __restrict__ body,
    const int32_t* __restrict__ leaf_off, int num_leaves, int qblocks, int cap, int32_t* __restrict__ leaf_fill,
    int32_t* __restrict__ pairs)
{
    const int qb = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (body[b].overflow) return;
    const int cnt = list_len[(size_t)b * qblocks + qb];
    const RayEntry* list = lists + ((size_t)b * qblocks + qb) * num_leaves;
    int32_t* out = pairs + (size_t)b * cap;
    for (int base = 0; base < cnt; base += 64) {
        // lanes over entries: reserve the entry's range in its leaf (64 atomics in flight)
        const int j = base + lane;
        RayEntry e = RayEntry{0, 0, 0u, 0u};
        int dst = 0;
        if (j < cnt) {
            e = list[j];
            const int n = __builtin_popcount(e.mask_lo) + __builtin_popcount(e.mask_hi);
            dst = leaf_off[(size_t)b * num_leaves + e.leaf] + atomicAdd(&leaf_fill[(size_t)b * num_leaves + e.leaf], n);
        }
        // lanes over rays: entry by entry, the set lanes write their slot
        const int m = min(64, cnt - base);
        for (int k = 0; k < m; ++k) {
            const uint32_t lo = __builtin_amdgcn_readlane(e.mask_lo, k), hi = __builtin_amdgcn_readlane(e.mask_hi, k);
            const int d = __builtin_amdgcn_readlane(dst, k);
            const unsigned long long mask = ((unsigned long long)hi << 32) | lo;
            if ((mask >> lane) & 1ull)
                out[d + __builtin_popcountll(mask & ((1ull << lane) - 1ull))] = qb * kRayQueries + lane;
        }
    }
}

// ray_tiles_kernel + ray_fill_kernel in one launch: kFillSplit one-wave workgroups per body.  Each scans the body's
// counts for itself (430 numbers, seven per lane and a wavefront scan); the first one writes the tile table; the body's
// entries -- all its query blocks' lists laid end to end through a prefix of their lengths -- are dealt out 64 at a time.
// (As two launches with one wavefront per query block: 10 + 31 us at batch 64 and 7 + 14 us at batch 8, most of it the
// launch rate of 6912 one-wavefront workgroups and three dependent global round trips in each; as ONE workgroup per body,
// fill counters in LDS: 61 us -- the write loop below is ~25 instructions per entry and a body's 4300 entries kept one CU
// busy that long.)
// ONE-wavefront workgroups: beside the nearest-vertex search -- 55 k one-wave workgroups that take every wave slot as it
// falls free -- a workgroup of four wavefronts waits until a CU has four free slots AT ONCE: the 256-thread form of
// this kernel took 24 us alone and 77-95 us in the replayed step, on the chain in front of the crossing kernel.
constexpr int kTilesFillBlock = 64, kFillSplit = 64, kFillMaxBlocks = 2048;
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}
__global__ __launch_bounds__(kTilesFillBlock) void ray_tiles_fill_kernel(
    const int32_t* __restrict__ leaf_cnt, const TreeNode* __restrict__ nodes, const int32_t* __restrict__ leaf_nodes,
    int num_leaves, int cap, int max_tiles, int fallback_tiles, RayTile* __restrict__ tiles, RayBody* __restrict__ body,
    const RayEntry* __restrict__ lists, const int32_t* __restrict__ list_len, int qblocks, int32_t* __restrict__ leaf_fill,
    int32_t* __restrict__ pairs, int list_stride)
{
    __builtin_amdgcn_s_setprio(3);                  // a chain of short dependent steps: ask for the issue slots first
    extern __shared__ int32_t dyn[];                // off[num_leaves] | tile[num_leaves] | blk[qblocks + 1]
    int32_t* off_s = dyn;
    int32_t* tile_s = dyn + num_leaves;
    int32_t* blk = dyn + 2 * num_leaves;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int per = (num_leaves + 63) / 64;
    const int l0 = min(lane * per, num_leaves), l1 = min(l0 + per, num_leaves);
    const int perq = (qblocks + 63) / 64;
    const int q0 = min(lane * perq, qblocks), q1 = min(q0 + perq, qblocks);
    const int32_t* cnt = leaf_cnt + (size_t)b * num_leaves;
    const int32_t* len = list_len + (size_t)b * qblocks;
    int npairs = 0, ntile = 0, nent = 0;
    for (int l = l0; l < l1; ++l) { const int c = cnt[l]; npairs += c; ntile += ray_tile_count(c); }
    for (int q = q0; q < q1; ++q) nent += len[q];
    const int sp = wave_inclusive_scan(npairs, lane), st = wave_inclusive_scan(ntile, lane), sq = wave_inclusive_scan(nent, lane);
    const int total_pairs = __builtin_amdgcn_readlane(sp, 63), total_tiles = __builtin_amdgcn_readlane(st, 63);
    const int total = __builtin_amdgcn_readlane(sq, 63);
    const bool overflow = total_pairs > cap || total_tiles > max_tiles;
    if (lane == 0 && blockIdx.y == 0) body[b] = RayBody{overflow ? fallback_tiles : total_tiles, overflow ? 1 : 0};
    if (overflow) return;
    {
        int off = sp - npairs, tile = st - ntile;
        for (int l = l0; l < l1; ++l) {
            const int c = cnt[l];
            off_s[l] = off;
            tile_s[l] = tile;
            off += c;
            tile += ray_tile_count(c);
        }
        int ent = sq - nent;
        for (int q = q0; q < q1; ++q) { blk[q] = ent; ent += len[q]; }
        if (lane == 0) blk[qblocks] = total;
    }
    __syncthreads();
    // the tile table: every workgroup of the body writes the tiles of a few leaves (one leaf per lane: two dependent loads
    // and a short loop) -- written by the body's first workgroup alone, seven leaves per lane one after the other, it was
    // the longest chain in the launch
    for (int l = (int)blockIdx.y + (int)gridDim.y * lane; l < num_leaves; l += (int)gridDim.y * 64) {
        const TreeNode nd = nodes[leaf_nodes[l]];
        const int ex_off = nd.ex_off, ex_len = nd.ex_len;
        const int c = cnt[l], off = off_s[l];
        RayTile* out = tiles + (size_t)b * max_tiles + tile_s[l];
        for (int k = 0; k < ray_tile_count(c); ++k) *out++ = ray_tile_at(ex_off, ex_len, off, c, k);
    }
    int32_t* fill = leaf_fill + (size_t)b * num_leaves;
    int32_t* out = pairs + (size_t)b * cap;
    for (int base = (int)blockIdx.y * 64; base < total; base += (int)gridDim.y * 64) {
        // lanes over entries: reserve the entry's range in its leaf (64 atomics in flight)
        const int g = base + lane;
        RayEntry e = RayEntry{0, 0, 0u, 0u};
        int dst = 0, qb = 0;
        if (g < total) {
            int lo = 0, hi = qblocks;                       // the block with blk[qb] <= g < blk[qb + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (blk[mid] <= g) lo = mid; else hi = mid;
            }
            qb = lo;
            e = lists[((size_t)b * qblocks + qb) * list_stride + (g - blk[qb])];
            dst = off_s[e.leaf] + atomicAdd(&fill[e.leaf], __builtin_popcount(e.mask_lo) + __builtin_popcount(e.mask_hi));
        }
        // lanes over rays: entry by entry, the set lanes write their slot
        const int m = min(64, total - base);
        for (int k = 0; k < m; ++k) {
            const uint32_t lo = __builtin_amdgcn_readlane(e.mask_lo, k), hi = __builtin_amdgcn_readlane(e.mask_hi, k);
            const int d = __builtin_amdgcn_readlane(dst, k), q = __builtin_amdgcn_readlane(qb, k);
            const unsigned long long mask = ((unsigned long long)hi << 32) | lo;
            if ((mask >> lane) & 1ull)
                out[d + __builtin_popcountll(mask & ((1ull << lane) - 1ull))] = q * kRayQueries + lane;
        }
    }
}

// Crossing counts, leaf-major: a wavefront takes a tile -- one leaf and up to 64 of the rays that pass its slabs,
// whichever query blocks they come from, and with a leaf's last full tile the up to 63 rays it has left over as a
// second set (see the walk's header) -- walks the leaf's strip run in one pass and adds each ray's crossings to its
// query's count.  (Block-major, 64 neighbouring queries against every leaf any of them meets, only ~22 % of the lanes
// can have a crossing at all: measured, tuch_ray_work.)  Queries: the model's vertices in tree order (qperm != nullptr;
// faces around the query are skipped) or arbitrary points [B,Q,3] in the caller's order.
// Grid (G = min(B, 8), workers): workgroups go round-robin to the 8 XCDs, so the wavefronts of column x all sit on one
// XCD; together they work through bodies x, x + G, x + 2 G, ... one after the other (a body's 0.2 MB sheared stream
// stays in that XCD's L2, and a body with many tiles is shared by all the column's wavefronts).
// The next tile (record, ray slot, query coordinates: a chain of dependent loads) is fetched while the current one is
// walked.  A body marked overflow is walked block-major: tile t = (query block t / 8, every 8th leaf of the block's
// list from t % 8).
// kCount: elements walked are added to stats[0] (measurement).
// kSeg (vertex queries of a model with segments): the crossings with the faces of the lane's own segments are counted
// as well (seg_count[b][slot][2], four signed byte counters per word; the elements' segments ride in the stream's
// fourth word -- tree_sign_word --, the vertices' in seg_vmask).
template <bool kVerts, bool kCount, bool kSeg>
__global__ __launch_bounds__(64) void ray_leaf_kernel(
    const float* __restrict__ pts, const RayElem* __restrict__ stream, const float4* __restrict__ boxes,
    const RayTile* __restrict__ tiles, const RayBody* __restrict__ body, const int32_t* __restrict__ pairs, const RayEntry* __restrict__ lists,
    const int32_t* __restrict__ list_len, const TreeNode* __restrict__ nodes, int num_leaves,
    const int32_t* __restrict__ qperm, const int32_t* __restrict__ counts, int Q, int T, int qblocks, int num_bodies,
    int cap, int max_tiles, int32_t* __restrict__ count, unsigned long long* __restrict__ stats,
    const int32_t* __restrict__ vmask, int32_t* __restrict__ seg_count)
{
    const int lane = threadIdx.x;
    // a lane's ray: its slot in the body's order, its segments (kSeg) and its sheared origin
    struct Ray { int slot, qmask; float qx, qy, qz; };
    // b < 0: nothing left; len < 0: block-major tile `off`; nb > 0 (wave-uniform): lanes below nb hold a ray of set B too,
    // slot_b, the point it starts from i_b
    struct Work { int b, off, len, nb; bool active; Ray ra; int slot_b, i_b; float4 pre; RayElem pre_el; };
    // The tiles of the column's bodies x, x + G, ... form one sequence; wavefront y takes every gridDim.y-th of it (a
    // work counter instead serialises: ~100 ns per atomic on one address, measured).
    int b_cur = blockIdx.x, base = 0, g = blockIdx.y;       // current body, tiles before it, next position in the sequence
    auto origin = [&](Ray& r, int b, int i) {
        const float* pb = pts + (size_t)b * Q * 3;
        r.qz = pb[3 * i + 2];
        r.qx = shear_x(pb[3 * i], r.qz);
        r.qy = shear_y(pb[3 * i + 1], r.qz);
        if (kSeg) r.qmask = vmask[r.slot];
    };
    auto fetch = [&]() {
        Work w;
        w.b = -1; w.off = w.len = w.nb = w.slot_b = w.i_b = 0; w.active = false;
        w.ra = Ray{0, 0, 0.0f, 0.0f, 0.0f};
        w.pre = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        w.pre_el = RayElem{0.0f, 0.0f, 0.0f, 0.0f};
        while (b_cur < num_bodies) {
            const int b = b_cur;
            const int nt = __builtin_amdgcn_readfirstlane(body[b].tiles);
            if (g >= base + nt) { base += nt; b_cur += gridDim.x; continue; }
            const int t = g - base;
            g += gridDim.y;
            w.b = b;
            int i0;
            if (!__builtin_amdgcn_readfirstlane(body[b].overflow)) {
                const RayTile tile = tiles[(size_t)b * max_tiles + t];
                const int n = __builtin_amdgcn_readfirstlane(tile.n), first = __builtin_amdgcn_readfirstlane(tile.first);
                w.active = lane < n;
                w.ra.slot = pairs[(size_t)b * cap + first + (w.active ? lane : 0)];
                i0 = kVerts ? qperm[w.ra.slot] : w.ra.slot;
                w.off = __builtin_amdgcn_readfirstlane(tile.ex_off);
                w.len = __builtin_amdgcn_readfirstlane(tile.ex_len);
                w.pre = boxes[(size_t)b * T + min(w.off + lane, T - 1)];      // the run's first chunk of boxes, one per lane
                w.pre_el = stream[(size_t)b * T + min(max(w.off - 2 + lane, 0), T - 1)];
                // set B, the leaf's remainder riding its last full tile: slot and point are fetched beside set A's (no
                // dependent round trip more); the coordinates follow when the pass begins and go to LDS, not into registers
                // held over the pass before
                w.nb = n - kRayQueries;
                if (w.nb > 0) {
                    w.slot_b = pairs[(size_t)b * cap + first + (lane < w.nb ? kRayQueries + lane : 0)];
                    w.i_b = kVerts ? qperm[w.slot_b] : w.slot_b;
                }
            } else {
                const int nq = kVerts ? Q : (counts ? counts[b] : Q);
                w.ra.slot = (t / kFallbackChunks) * kRayQueries + lane;
                w.active = w.ra.slot < nq;
                i0 = kVerts ? qperm[w.ra.slot] : min(w.ra.slot, nq - 1);
                w.off = t;                     // block-major tile: (query block, chunk) packed, marked by len < 0; one set
                w.len = -1;
            }
            origin(w.ra, b, i0);
            break;
        }
        return w;
    };
    int walked = 0;
    __shared__ RayQueue queue;
    queue.cross[lane] = 0; queue.cross[lane + 64] = 0;
    queue.seg[0][lane] = 0u; queue.seg[1][lane] = 0u;
    queue.seg[0][lane + 64] = 0u; queue.seg[1][lane + 64] = 0u;
    queue.ring[lane] = 0u; queue.ring[lane + 64] = 0u;
    uint32_t head = 0u, tail = 0u;                          // wave-uniform; tail - head = entries queued
    Work next = fetch();
    while (next.b >= 0) {
        const Work w = next;
        RayLane me;
        me.qx = w.ra.qx; me.qy = w.ra.qy; me.qz = w.ra.qz; me.qmask = w.ra.qmask; me.active = w.active;
        me.two = w.nb > 0;
        me.active_b = lane < w.nb;
        if (me.two) {
            Ray rb;
            rb.slot = w.slot_b; rb.qmask = 0;
            origin(rb, w.b, w.i_b);
            queue.org_b[lane] = make_float4(rb.qx, rb.qy, rb.qz, __int_as_float(rb.qmask));
        }
        if (w.len >= 0) ray_stage(queue, lane, w.pre, w.pre_el);
        next = fetch();
        RaySums sa = {0, 0u, 0u}, sb = {0, 0u, 0u};
        const RayElem* st = stream + (size_t)w.b * T;
        const float4* bx = boxes + (size_t)w.b * T;
        if (w.len >= 0) {
            ray_run<kVerts, kSeg>(st, bx, w.off, w.len, T, queue, head, tail, me, lane, true);
            if (kCount) walked += w.len;
        } else {
            const int qb = w.off / kFallbackChunks, c = w.off % kFallbackChunks;
            const int cnt = __builtin_amdgcn_readfirstlane(list_len[(size_t)w.b * qblocks + qb]);
            const RayEntry* list = lists + ((size_t)w.b * qblocks + qb) * num_leaves;
            for (int j = c; j < cnt; j += kFallbackChunks) {
                const TreeNode nd = nodes[__builtin_amdgcn_readfirstlane(list[j].node)];
                ray_run<kVerts, kSeg>(st, bx, nd.ex_off, nd.ex_len, T, queue, head, tail, me, lane, false);
                if (kCount) walked += nd.ex_len;
            }
        }
        // (the queue is emptied per pass: its entries name lanes of THIS pass's rays and elements of this pass's body)
        ray_flush<kVerts, kSeg>(queue, head, tail, me, lane, sa, sb);
        auto add = [&](const RaySums& s, int slot) {
            if (s.crossings != 0) atomicAdd(&count[((size_t)w.b * qblocks) * kRayQueries + slot], s.crossings);
            if (kSeg && (s.pa != 0u || s.pb != 0u)) {                             // few lanes
                // two words of four byte-wide counters per ray; a pass's byte sums are added as ONE integer: the
                // running word may borrow across its bytes, the final word is the exact sum all the same (seg_leaf_count)
                int32_t* sc = seg_count + 2 * (((size_t)w.b * qblocks) * kRayQueries + slot);
                if (s.pa != 0u) atomicAdd(sc, (int32_t)s.pa);
                if (s.pb != 0u) atomicAdd(sc + 1, (int32_t)s.pb);
            }
        };
        if (w.active) add(sa, w.ra.slot);
        if (me.active_b) add(sb, w.slot_b);
    }
    if (kCount && lane == 0) atomicAdd(stats, (unsigned long long)walked);
}

// atan2 with a degree-8 minimax atan on [0,1] (max abs error 1e-7), octant fix-up; atan2(0,0) = 0
__device__ __forceinline__ float fast_atan2(float y, float x)
{
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const float mx = __builtin_fmaxf(__builtin_fmaxf(ax, ay), 1e-37f);
    const float t = __builtin_fminf(ax, ay) / mx;
    const float s = t * t;
    float p = 0.0024567253421992064f;
    p = p * s + -0.014401361346244812f;
    p = p * s + 0.03978123143315315f;
    p = p * s + -0.07234857976436615f;
    p = p * s + 0.10498946160078049f;
    p = p * s + -0.14161229133605957f;
    p = p * s + 0.19985906779766083f;
    p = p * s + -0.33332598209381104f;
    p = p * s + 0.9999998807907104f;
    float v = p * t;
    v = ay > ax ? 1.57079632679489661923f - v : v;
    v = x < 0.0f ? kPi - v : v;
    return __builtin_copysignf(v, y);
}

// half solid angle atan2(num, den) of the triangle with corner vectors a, b, c (contact.py:79-105)
__device__ __forceinline__ float half_solid_angle(const P3& a, const P3& b, const P3& c)
{
    const float na = __builtin_sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
    const float nb = __builtin_sqrtf(b.x * b.x + b.y * b.y + b.z * b.z);
    const float nc = __builtin_sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
    const float cx = b.y * c.z - b.z * c.y, cy = b.z * c.x - b.x * c.z, cz = b.x * c.y - b.y * c.x;
    const float num = a.x * cx + a.y * cy + a.z * cz;
    const float dab = a.x * b.x + a.y * b.y + a.z * b.z;
    const float dbc = b.x * c.x + b.y * c.y + b.z * c.z;
    const float dac = a.x * c.x + a.y * c.y + a.z * c.z;
    const float den = na * nb * nc + dab * nc + dac * nb + dbc * na;
    return fast_atan2(num, den);
}

// One cone triangle (apex direction u, then x, y) of a closing fan / closing chain: its signed ray crossing and its half
// solid angle, BOTH signed by ONE determinant.  The two only mean something together: where u comes to lie in the plane
// of (query, x, y) -- a fan direction tangent to a face of the star -- the crossing flips by one and the half angle
// jumps by 2 pi / 2, and crossing - half / (2 pi) is continuous across the flip.  Computing det(u, x, y) twice (sheared
// for the crossing, unsheared inside the angle; equal in exact arithmetic, the shear has determinant 1) let the two
// signs disagree when the determinant is within rounding of zero: w off by exactly one, about once in 3 million cone
// triangles (found on the irregular-topology body, tests/test_gpu_contact.py::test_big_batches_...).  Exactly zero counts
// as positive for both.  s*: corners relative to the query in the sheared ray frame; u, pb, pc: the same in space.
__device__ __forceinline__ void cone_term(const P3& us, const P3& sb, const P3& sc, const P3& u, const P3& pb, const P3& pc,
                                          int& crossings, float& half)
{
    const float ea = edge_fn(sb, sc), eb = edge_fn(sc, us), ec = edge_fn(us, sb);
    const float d = ea * us.z + eb * sb.z + ec * sc.z;
    const bool la = left_of(ea, sb, sc), lb = left_of(eb, sc, us), lc = left_of(ec, us, sb);
    const bool front = d >= 0.0f;
    crossings = (la & lb & lc) ? (int)front : ((!la & !lb & !lc) ? -(int)!front : 0);
    const float nu = __builtin_sqrtf(u.x * u.x + u.y * u.y + u.z * u.z);
    const float nb = __builtin_sqrtf(pb.x * pb.x + pb.y * pb.y + pb.z * pb.z);
    const float nc = __builtin_sqrtf(pc.x * pc.x + pc.y * pc.y + pc.z * pc.z);
    const float cx = pb.y * pc.z - pb.z * pc.y, cy = pb.z * pc.x - pb.x * pc.z, cz = pb.x * pc.y - pb.y * pc.x;
    const float num = __builtin_fabsf(u.x * cx + u.y * cy + u.z * cz);
    const float dub = u.x * pb.x + u.y * pb.y + u.z * pb.z;
    const float dbc = pb.x * pc.x + pb.y * pc.y + pb.z * pc.z;
    const float duc = u.x * pc.x + u.y * pc.y + u.z * pc.z;
    const float den = nu * nb * nc + dub * nc + duc * nb + dbc * nu;
    half = fast_atan2(front ? num : -num, den);
}

// The closing fan of a VERTEX: n += its signed crossings, returns the sum of its half angles.  w = N - half_sum / (2 pi),
// N = count + crossings of the fan (fan_winding below).
// One vertex per lane (`real` = false: a padding lane; all lanes of the wavefront must call -- long rings are shared out).
__device__ __forceinline__ float fan_terms(const float* __restrict__ vb, int v, bool real, int& n,
                                           const int32_t* __restrict__ ring_off, const int32_t* __restrict__ ring_vidx)
{
    const float vx = vb[3 * v], vy = vb[3 * v + 1], vz = vb[3 * v + 2];
    const float qx = shear_x(vx, vz), qy = shear_y(vy, vz);
    // the apex direction of the fan, in space and sheared (ray frame)
    const P3 u_dir = {kFanX, kFanY, kFanZ};
    const P3 us = {shear_x(kFanX, kFanZ), shear_y(kFanY, kFanZ), kFanZ};
    const int lo = ring_off[v], cnt = real ? ring_off[v + 1] - lo : 0;
    float half_sum = 0.0f;
    constexpr int kLongRing = 16;
    constexpr int kShortRing = 8;
    if (cnt > 0 && cnt <= kShortRing) {
        // the usual case (SMPL: valence 6, a few 7 - 9): ALL ring vertices' ids in one round of loads, all their coordinates
        // in the next -- with four at a time and the cycle's last vertex first this was six dependent rounds
        int rr[kShortRing];
        float cc[kShortRing][3];
#pragma unroll
        for (int u = 0; u < kShortRing; ++u) rr[u] = ring_vidx[lo + min(u, cnt - 1)];
#pragma unroll
        for (int u = 0; u < kShortRing; ++u) { cc[u][0] = vb[3 * rr[u]]; cc[u][1] = vb[3 * rr[u] + 1]; cc[u][2] = vb[3 * rr[u] + 2]; }
        // slots behind the ring repeat its last vertex: slot kShortRing - 1 always holds the cycle's predecessor of vertex 0
        P3 pb = {cc[kShortRing - 1][0] - vx, cc[kShortRing - 1][1] - vy, cc[kShortRing - 1][2] - vz};
        P3 sb = {shear_x(cc[kShortRing - 1][0], cc[kShortRing - 1][2]) - qx, shear_y(cc[kShortRing - 1][1], cc[kShortRing - 1][2]) - qy,
                 cc[kShortRing - 1][2] - vz};
#pragma unroll
        for (int u = 0; u < kShortRing; ++u) {
            if (u < cnt) {
                const P3 pc = {cc[u][0] - vx, cc[u][1] - vy, cc[u][2] - vz};
                const P3 sc = {shear_x(cc[u][0], cc[u][2]) - qx, shear_y(cc[u][1], cc[u][2]) - qy, cc[u][2] - vz};
                int cr;
                float hf;
                cone_term(us, sb, sc, u_dir, pb, pc, cr, hf);
                half_sum += hf;
                n += cr;
                pb = pc;
                sb = sc;
            }
        }
    } else if (cnt > 0 && cnt <= kLongRing) {
        // previous ring vertex (j = cnt-1) to start the cycle
        int r = ring_vidx[lo + cnt - 1];
        P3 pb = {vb[3 * r] - vx, vb[3 * r + 1] - vy, vb[3 * r + 2] - vz};
        P3 sb = {shear_x(vb[3 * r], vb[3 * r + 2]) - qx, shear_y(vb[3 * r + 1], vb[3 * r + 2]) - qy, vb[3 * r + 2] - vz};
        // four ring vertices at a time: their ids, then their coordinates, are fetched together (the loop is
        // otherwise a chain of dependent gathers: id -> coordinates -> next id ...)
        for (int j0 = 0; j0 < cnt; j0 += 4) {
            int rr[4];
            float cc[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) rr[u] = ring_vidx[lo + min(j0 + u, cnt - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) { cc[u][0] = vb[3 * rr[u]]; cc[u][1] = vb[3 * rr[u] + 1]; cc[u][2] = vb[3 * rr[u] + 2]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (j0 + u < cnt) {
                    const P3 pc = {cc[u][0] - vx, cc[u][1] - vy, cc[u][2] - vz};
                    const P3 sc = {shear_x(cc[u][0], cc[u][2]) - qx, shear_y(cc[u][1], cc[u][2]) - qy, cc[u][2] - vz};
                    int cr;
                    float hf;
                    cone_term(us, sb, sc, u_dir, pb, pc, cr, hf);
                    half_sum += hf;
                    n += cr;
                    pb = pc;
                    sb = sc;
                }
            }
        }
    }
    // long rings (the poles of a lat-long sphere; SMPL has none above 16) are shared out over the wavefront: one fan
    // triangle per lane, sums by butterfly -- one lane walking 80 triangles would hold up the whole launch
    unsigned long long todo = __builtin_amdgcn_ballot_w64(cnt > kLongRing);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int llo = __builtin_amdgcn_readlane(lo, src), lcnt = __builtin_amdgcn_readlane(cnt, src);
        const float lvx = __shfl(vx, src), lvy = __shfl(vy, src), lvz = __shfl(vz, src);
        float h = 0.0f;
        int cr = 0;
        for (int j = lane; j < lcnt; j += 64) {
            const int r_prev = ring_vidx[llo + (j == 0 ? lcnt - 1 : j - 1)], r_cur = ring_vidx[llo + j];
            const float bx = vb[3 * r_prev], by = vb[3 * r_prev + 1], bz = vb[3 * r_prev + 2];
            const float cx = vb[3 * r_cur], cy = vb[3 * r_cur + 1], cz = vb[3 * r_cur + 2];
            const float lqx = shear_x(lvx, lvz), lqy = shear_y(lvy, lvz);
            const P3 pb = {bx - lvx, by - lvy, bz - lvz}, pc = {cx - lvx, cy - lvy, cz - lvz};
            const P3 sb = {shear_x(bx, bz) - lqx, shear_y(by, bz) - lqy, bz - lvz}, sc = {shear_x(cx, cz) - lqx, shear_y(cy, cz) - lqy, cz - lvz};
            int c1;
            float h1;
            cone_term(us, sb, sc, u_dir, pb, pc, c1, h1);
            h += h1;
            cr += c1;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { h += __shfl_xor(h, m); cr += __shfl_xor(cr, m); }
        if (lane == src) { half_sum = h; n += cr; }
    }
    return half_sum;
}
__device__ __forceinline__ float fan_winding(const float* __restrict__ vb, int v, bool real, int n,
                                             const int32_t* __restrict__ ring_off, const int32_t* __restrict__ ring_vidx)
{
    const float half_sum = fan_terms(vb, v, real, n, ring_off, ring_vidx);
    return (float)n - half_sum * (0.5f / kPi);
}

// vertices: the body test's flags from the crossing counts
__global__ __launch_bounds__(kBlock) void ray_finalize_verts_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ count, const int32_t* __restrict__ qperm,
    const int32_t* __restrict__ ring_off, const int32_t* __restrict__ ring_vidx,
    int V, int stride, float thresh, float* __restrict__ w_out, uint8_t* __restrict__ exterior,
    uint8_t* __restrict__ exterior_copy)                 // or nullptr: the same flags once more (the two-launch segment
                                                         // filter reads them while it re-marks `exterior`)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;     // position in tree order
    const bool real = i < V;                             // all lanes stay: long rings need the whole wavefront
    const int v = qperm[real ? i : V - 1];
    const int n = count[(size_t)b * stride + (real ? i : V - 1)];
    const float w = fan_winding(verts + (size_t)b * V * 3, v, real, n, ring_off, ring_vidx);
    const size_t o = (size_t)b * V + v;
    if (real) {
        if (w_out) w_out[o] = w;
        if (exterior) exterior[o] = w <= thresh;
        if (exterior_copy) exterior_copy[o] = w <= thresh;
    }
}

__global__ __launch_bounds__(kBlock) void ray_finalize_points_kernel(
    const int32_t* __restrict__ count, const int32_t* __restrict__ counts,
    int Q, int stride, float thresh, float* __restrict__ w_out, uint8_t* __restrict__ exterior)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= Q) return;
    const int n = (!counts || i < counts[b]) ? count[(size_t)b * stride + i] : 0;
    const float w = (float)n;
    const size_t o = (size_t)b * Q + i;
    if (w_out) w_out[o] = w;
    if (exterior) exterior[o] = w <= thresh;
}

// ---- the segment filter by ray crossings ------------------------------------------------------------------------
// has_self_isect (segmentation.py:81-99): winding number of a segment's vertices w.r.t. its own "closed" mesh T
// (segment faces + cap fans).  The reference sums the solid angles of the faces that do not contain the query v
// (the others are atan2(0,0) = 0): of the chain T' = T minus star(v).  Close T' with cones from its boundary to an
// apex v + delta u: the result is a 2-cycle, its winding number around v is the signed number of ray crossings, so
//     w_ref(v) = crossings(T') + sum over the closing chain C of [crossing - half angle / 2 pi] of the cone triangle,
//     C = -boundary(T') = links of star(v) - boundary(T),
// exactly the fan of the body test when T is a closed manifold (boundary(T) = 0, the links form the ring) -- but with no
// such assumption: the reference's caps need not close the segment consistently (segmentation.py:56-66 takes the loops
// as the asset lists them), and the synthetic segments do leave a few dozen boundary edges.  As for the fan, the cone
// terms depend on the direction u only.  A segment vertex on no face of its segment has no links: w = crossings - the
// boundary terms.
// The segment meshes are small (hundreds of faces) and the queries few (the segment's interior vertices, compacted
// by winding.hip), so the layout is that of the solid-angle kernel it replaces: one wavefront per 64 queries and
// face split, triangles staged through LDS; ~30 plain operations per (query, triangle) instead of ~90.
constexpr int kSegRayChunk = 128;     // triangles staged in LDS per pass

// The entries a segment's crossing kernel walks, posed and sheared, 9 floats each: a face (three corners; index < V ->
// body vertex, else cap vertex, segmentation.py:77) or a boundary edge x -> y of the segment mesh with its (negative)
// multiplicity: [x', y', multiplicity, marker, 0].
constexpr float kConeMarker = 3.0e38f;
__global__ __launch_bounds__(kBlock) void segment_shear_entries_kernel(
    const float* __restrict__ verts, const float* __restrict__ caps,
    const int32_t* __restrict__ ent, int V, int K, int E, float* __restrict__ out)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= E) return;
    const int id[3] = {ent[3 * i], ent[3 * i + 1], ent[3 * i + 2]};
    float* dst = out + ((size_t)b * E + i) * 9;
    const int corners = id[2] < 0 ? 2 : 3;
    for (int k = 0; k < corners; ++k) {
        const float* src = id[k] < V ? verts + ((size_t)b * V + id[k]) * 3 : caps + ((size_t)b * K + (id[k] - V)) * 3;
        dst[3 * k] = shear_x(src[0], src[2]); dst[3 * k + 1] = shear_y(src[1], src[2]); dst[3 * k + 2] = src[2];
    }
    if (corners == 2) { dst[6] = (float)id[2]; dst[7] = kConeMarker; dst[8] = 0.0f; }
}

// Work items of the crossing kernel: (body, segment, block of 64 compacted queries), only those that exist -- a grid
// over the worst case (every segment vertex interior) is ten times larger and costs more in dispatch than in work.
// One workgroup; items[i] = (body * S + segment, first query), items_total[0] = how many, items_total[1] = face splits.
constexpr int kItemsBlock = 256;
__global__ __launch_bounds__(kItemsBlock) void segment_items_kernel(
    const int32_t* __restrict__ count, int BS, int2* __restrict__ items, int32_t* __restrict__ items_total,
    int max_split, int grid)
{
    __shared__ int sc[kItemsBlock];
    __shared__ int base;
    const int t = threadIdx.x;
    if (t == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < BS; c0 += kItemsBlock) {
        const int e = c0 + t;
        const int nb = e < BS ? (count[e] + 63) >> 6 : 0;
        sc[t] = nb;
        __syncthreads();
        for (int d = 1; d < kItemsBlock; d <<= 1) {          // inclusive scan
            const int add = t >= d ? sc[t - d] : 0;
            __syncthreads();
            sc[t] += add;
            __syncthreads();
        }
        const int off = base + sc[t] - nb;
        for (int k = 0; k < nb; ++k) items[off + k] = make_int2(e, 64 * k);
        __syncthreads();
        if (t == kItemsBlock - 1) base += sc[t];
        __syncthreads();
    }
    if (t == 0) {
        items_total[0] = base;
        // as many face splits as keep (items x splits) within 7/8 of one round of the crossing kernel's grid: a second,
        // mostly empty round cost more than the longer loops of fewer splits (16 splits: 110.3, 12: 112.1 k it/s at batch 64)
        const int fit = base > 0 ? (grid - grid / 8) / base : max_split;
        items_total[1] = fit < 1 ? 1 : (fit > max_split ? max_split : fit);
    }
}

__global__ __launch_bounds__(64) void segment_ray_kernel(
    const float* __restrict__ verts, const float* __restrict__ entries,
    const int2* __restrict__ items, const int32_t* __restrict__ items_total, const int32_t* __restrict__ seg_q_off,
    const int32_t* __restrict__ seg_q_vidx, const int32_t* __restrict__ ent_off,
    const int32_t* __restrict__ count, const int32_t* __restrict__ list, int V, int E,
    int Qs_total, int S, int nsplit, int32_t* __restrict__ partial,     // [B,nsplit,Qs_total] by list position: crossings
    float* __restrict__ partial_half)                                   // same shape: half angles of the boundary cones
{
    const P3 u_dir = {kFanX, kFanY, kFanZ};
    const P3 us = {shear_x(kFanX, kFanZ), shear_y(kFanY, kFanZ), kFanZ};
    __shared__ float sT[kSegRayChunk * 9];
    const int ns = items_total[1];                                      // face splits in use (<= nsplit, the array stride)
    const int units = items_total[0] * ns;                              // (item, face split)
    for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int2 item = items[unit / ns];
        const int split = unit % ns;
        const int b = item.x / S, s = item.x % S, k_start = item.y;
        const int n = count[item.x];
        const int q_beg = seg_q_off[s];
        const int32_t* mine = list + (size_t)b * Qs_total + q_beg;
        const int k0 = k_start + threadIdx.x;
        const int v0 = seg_q_vidx[q_beg + mine[min(k0, n - 1)]];
        const float* vb = verts + (size_t)b * V * 3;
        const float qz = vb[3 * v0 + 2];
        const float qx = shear_x(vb[3 * v0], qz), qy = shear_y(vb[3 * v0 + 1], qz);
        const int f_seg = ent_off[s], f_cnt = ent_off[s + 1] - f_seg;
        const int per = (f_cnt + ns - 1) / ns;
        const int f_beg = f_seg + split * per, f_end = min(f_seg + f_cnt, f_beg + per);
        int crossings = 0;
        float half_sum = 0.0f;
        for (int chunk = f_beg; chunk < f_end; chunk += kSegRayChunk) {
            const int cn = min(kSegRayChunk, f_end - chunk);
            const float* src = entries + ((size_t)b * E + chunk) * 9;
            __syncthreads();
            for (int i = threadIdx.x; i < cn * 9; i += 64) sT[i] = src[i];
            __syncthreads();
            for (int f = 0; f < cn; ++f) {
                const float* t = sT + f * 9;
                if (t[7] != kConeMarker) {                              // a face (wave-uniform: LDS broadcast)
                    const P3 a = {t[0] - qx, t[1] - qy, t[2] - qz}, bb = {t[3] - qx, t[4] - qy, t[5] - qz}, c = {t[6] - qx, t[7] - qy, t[8] - qz};
                    const float ea = edge_fn(bb, c), eb = edge_fn(c, a), ec = edge_fn(a, bb);
                    const float numz = ea * a.z + eb * bb.z + ec * c.z;
                    const float mn = __builtin_fminf(__builtin_fminf(ea, eb), ec), mx = __builtin_fmaxf(__builtin_fmaxf(ea, eb), ec);
                    int n1 = (int)(__builtin_fminf(mn, numz) > 0.0f) - (int)(__builtin_fmaxf(mx, numz) < 0.0f);
                    // exact ties with a definite depth; the faces around the query (det exactly 0) count 0 above
                    const bool edge_zero = mn * mx == 0.0f;
                    if (__builtin_amdgcn_ballot_w64(edge_zero)) {
                        const bool tie = edge_zero & (numz != 0.0f);
                        if (__builtin_amdgcn_ballot_w64(tie)) {
                            if (tie) n1 = crossing_with_ties<true>(a, bb, c, ea, eb, ec);
                        }
                    }
                    crossings += n1;
                } else {
                    // a boundary edge x -> y: the cone triangle (u, x, y), its apex a direction; edges at the query
                    // itself cancel against the spokes of its star and are left out
                    const P3 bb = {t[0] - qx, t[1] - qy, t[2] - qz}, c = {t[3] - qx, t[4] - qy, t[5] - qz};
                    const bool at_query = ((bb.x == 0.0f) & (bb.y == 0.0f) & (bb.z == 0.0f)) | ((c.x == 0.0f) & (c.y == 0.0f) & (c.z == 0.0f));
                    if (!at_query) {
                        const int mult = (int)t[6];
                        // back from the sheared frame for the angle
                        const P3 pb = {__builtin_fmaf(kShearX, bb.z, bb.x), __builtin_fmaf(kShearY, bb.z, bb.y), bb.z};
                        const P3 pc = {__builtin_fmaf(kShearX, c.z, c.x), __builtin_fmaf(kShearY, c.z, c.y), c.z};
                        int c1;
                        float h1;
                        cone_term(us, bb, c, u_dir, pb, pc, c1, h1);
                        crossings += mult * c1;
                        half_sum += (float)mult * h1;
                    }
                }
            }
        }
        const size_t o = ((size_t)b * nsplit + split) * Qs_total + q_beg;
        if (k0 < n) { partial[o + k0] = crossings; partial_half[o + k0] = half_sum; }
    }
}

// counter s (0..7) of a ray's two packed words: the words are sums of signed per-byte contributions (|total| < 128 per
// byte), so the bytes are peeled off from the low end, each one's sign carried into the rest
__device__ __forceinline__ int seg_leaf_count(const int32_t* words, int s)
{
    int32_t x = words[s >> 2];
    int c = 0;
    for (int k = 0; k <= (s & 3); ++k) {
        c = (int)(int8_t)(x & 255);
        x = (x - c) >> 8;
    }
    return c;
}

// vertices that are NOT exterior to their own segment are re-marked exterior in the body flags
// (losses.py:87-89, loss.py:265-266)
__global__ __launch_bounds__(kBlock) void segment_ray_finalize_kernel(
    const float* __restrict__ verts, const float* __restrict__ caps, const int32_t* __restrict__ partial,
    const float* __restrict__ partial_half,
    const int32_t* __restrict__ seg_of_q, const int32_t* __restrict__ seg_q_off, const int32_t* __restrict__ seg_q_vidx,
    const int32_t* __restrict__ link_off, const int32_t* __restrict__ link,
    const int32_t* __restrict__ count, const int32_t* __restrict__ list,
    const int32_t* __restrict__ leaf_counts,      // [B][slots][2] crossings with the segments' body faces, or nullptr
    const int32_t* __restrict__ vpos, int slots, int V, int K,
    int Qs_total, int S, int nsplit, const int32_t* __restrict__ items_total, float thresh, float* __restrict__ seg_w,
    uint8_t* __restrict__ seg_ext, uint8_t* __restrict__ exterior)
{
    const int b = blockIdx.y;
    const int q = blockIdx.x * kBlock + threadIdx.x;       // a list position
    const int ns = items_total[1];                         // face splits the crossing kernel used (<= nsplit, the stride)
    // all lanes stay to the end: long link lists below are shared out over the wavefront
    bool active = q < Qs_total;
    const int s = active ? seg_of_q[q] : 0;
    const int k = q - seg_q_off[s];
    active = active && k < count[b * S + s];
    int n = 0;
    float half_sum = 0.0f;
    int qq = 0, v = 0;
    if (active) {
        for (int sp = 0; sp < ns; ++sp) {
            n += partial[((size_t)b * nsplit + sp) * Qs_total + q];
            half_sum += partial_half[((size_t)b * nsplit + sp) * Qs_total + q];
        }
        qq = seg_q_off[s] + list[(size_t)b * Qs_total + q];   // the vertex's slot in the segment tables
        v = seg_q_vidx[qq];
        if (leaf_counts) n += seg_leaf_count(leaf_counts + 2 * ((size_t)b * slots + vpos[v]), s);
    }
    const float* vb = verts + (size_t)b * V * 3;
    const float* cb = caps + (size_t)b * K * 3;
    const float vx = vb[3 * v], vy = vb[3 * v + 1], vz = vb[3 * v + 2];
    const float qx = shear_x(vx, vz), qy = shear_y(vy, vz);
    const P3 u_dir = {kFanX, kFanY, kFanZ};
    const P3 us = {shear_x(kFanX, kFanZ), shear_y(kFanY, kFanZ), kFanZ};
    // cone triangle (apex direction u, x, y) of one link x -> y of a vertex's star
    auto cone = [&](const float* p0, const float* p1, float ax, float ay, float az, float sx, float sy, float& h, int& c) {
        const P3 pb = {p0[0] - ax, p0[1] - ay, p0[2] - az}, pc = {p1[0] - ax, p1[1] - ay, p1[2] - az};
        const P3 sb = {shear_x(p0[0], p0[2]) - sx, shear_y(p0[1], p0[2]) - sy, p0[2] - az};
        const P3 sc = {shear_x(p1[0], p1[2]) - sx, shear_y(p1[1], p1[2]) - sy, p1[2] - az};
        int c1;
        float h1;
        cone_term(us, sb, sc, u_dir, pb, pc, c1, h1);
        h += h1;
        c += c1;
    };
    const int e0 = active ? link_off[qq] : 0, e1 = active ? link_off[qq + 1] : 0;
    constexpr int kLongLinks = 16;
    if (e1 - e0 <= kLongLinks) {
        // two links at a time (their four corner positions are fetched together)
        for (int e = e0; e < e1; e += 2) {
            int id[4];
            float pp[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) id[u] = link[2 * min(e + (u >> 1), e1 - 1) + (u & 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* p = id[u] < V ? vb + 3 * (size_t)id[u] : cb + 3 * (size_t)(id[u] - V);
                pp[u][0] = p[0]; pp[u][1] = p[1]; pp[u][2] = p[2];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (e + h < e1) cone(pp[2 * h], pp[2 * h + 1], vx, vy, vz, qx, qy, half_sum, n);
        }
    }
    // long stars (the poles of a lat-long sphere have 80 links; SMPL has none above 16): one link per lane, sums by
    // butterfly -- one lane walking 80 cones alone held the whole launch up (14 us or 50, depending on whether a pole
    // was interior in that iteration)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(e1 - e0 > kLongLinks);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int le0 = __builtin_amdgcn_readlane(e0, src), le1 = __builtin_amdgcn_readlane(e1, src);
        const float lvx = __shfl(vx, src), lvy = __shfl(vy, src), lvz = __shfl(vz, src);
        const float lqx = __shfl(qx, src), lqy = __shfl(qy, src);
        float h = 0.0f;
        int cr = 0;
        for (int e = le0 + lane; e < le1; e += 64) {
            const int i0 = link[2 * e], i1 = link[2 * e + 1];
            const float* p0 = i0 < V ? vb + 3 * (size_t)i0 : cb + 3 * (size_t)(i0 - V);
            const float* p1 = i1 < V ? vb + 3 * (size_t)i1 : cb + 3 * (size_t)(i1 - V);
            const float a0[3] = {p0[0], p0[1], p0[2]}, a1[3] = {p1[0], p1[1], p1[2]};
            cone(a0, a1, lvx, lvy, lvz, lqx, lqy, h, cr);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { h += __shfl_xor(h, m); cr += __shfl_xor(cr, m); }
        if (lane == src) { half_sum += h; n += cr; }
    }
    if (!active) return;
    const float w = (float)n - half_sum * (0.5f / kPi);
    const size_t o = (size_t)b * Qs_total + qq;
    if (seg_w) seg_w[o] = w;
    if (seg_ext) seg_ext[o] = w <= thresh;
    if (exterior && !(w <= thresh)) exterior[(size_t)b * V + v] = 1;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct RayLayout {
    size_t stream, boxes, bounds, lists, list_len, zeroed, zeroed_bytes, leaf_cnt, leaf_fill, count, leaf_off, tiles, body, pairs,
        stats, total;
    int T, qblocks, cap, max_tiles, workers, columns;
    size_t seg_count;        // per-segment crossing counts of the vertices (models with seg_elem_mask), zeroed with `count`
};

// ---- the segment filter behind the body test (flags only, leaf-assisted models) ------------------------------------------
// cap centroids -> sheared entries -> compaction of the interior vertices -> work items -> crossings -> cones + flags were
// six launches in round 2 (two ahead of the body test, four behind it: ~60 us of the step's serial chain at batch 64 for a
// few hundred interior vertices per body), two in round 3 (segment_cross_kernel: one workgroup per (segment, body, 1/16 of
// the entries), partial sums to global memory; segment_flags_kernel: sums + cones + flags: 48 + 18 us), one since round 4.
constexpr int kSegFusedMaxQ = 4096;      // vertices of one segment (the synthetic head: ~1150)
constexpr int kSegFusedMaxCaps = 8;

// cap centroids of the caps c_lo .. c_hi -> s_caps (segmentation.py:74-76), a wavefront per cap
template <int kWaves>
__device__ __forceinline__ void seg_fused_caps(const float* __restrict__ vb, const int32_t* __restrict__ cap_off,
                                               const int32_t* __restrict__ cap_vidx, int c_lo, int c_hi, float* s_caps)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = c_lo + wave; c < c_hi; c += kWaves) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        const int beg = cap_off[c], end = cap_off[c + 1];
        for (int k = beg + lane; k < end; k += 64) {
            const float* p = vb + 3 * cap_vidx[k];
            sx += p[0]; sy += p[1]; sz += p[2];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sx += __shfl_down(sx, o, 64); sy += __shfl_down(sy, o, 64); sz += __shfl_down(sz, o, 64); }
        if (lane == 0) {
            const float inv = 1.0f / (float)(end - beg);
            s_caps[3 * (c - c_lo)] = sx * inv; s_caps[3 * (c - c_lo) + 1] = sy * inv; s_caps[3 * (c - c_lo) + 2] = sz * inv;
        }
    }
}

// ---- ONE launch (round 4) ---------------------------------------------------------------------------------------------
// In the two launches of round 3 every one of the 16 slice workgroups of a (segment, body) compacted the segment's interior
// vertices again, and the slices' sums travelled through global memory to the second launch.  Here kSegOneZ workgroups of eight wavefronts share a (segment, body) by VERTICES, not by entries:
//   A. the segment's interior vertices by the body test's flags (the copy nobody writes), compacted in list order -- the
//      same list in every workgroup; workgroup z owns the groups of 64 of them with index = z (mod kSegOneZ); none -> done;
//   B. the cap centroids;
//   C. ALL entries of the segment (cap faces, boundary edges), posed and sheared 256 at a time in LDS; the wavefronts share
//      out (own group) x (sub-slice of the entries): one group -> eight sub-slices, eight groups -> one each; lane = vertex,
//      entries by LDS broadcast; the sub-slices' sums meet in LDS;
//   D. per own interior vertex: those sums in sub-slice order + the crossings with the segment's body faces the body's own
//      inside test has counted (seg_leaf_count) + the cones of its links -> w; not exterior to its own segment ->
//      exterior[v] = 1 (losses.py:87-89, loss.py:265-266).
// Nothing crosses workgroups: no partial sums in global memory, no arrival counter, no second launch.
// (Measured on the way, solo at batch 64, against 63 us for the two launches: one workgroup per (segment, body) with four
// wavefronts, round 3: 81 us; 128 vertices per workgroup with the body winding numbers recomputed from the crossing counts
// so that nothing waits for the flags: 89 us -- interior vertices are scattered over a segment's list, every chunk that
// holds one walks all entries with a handful of live lanes; one workgroup of SIXTEEN wavefronts: 44 us at every batch size --
// a body whose arm lies in its trunk keeps one compute unit busy with ~80 k instructions; four workgroups sharing the
// ENTRIES with the last arrival finishing (partial sums + fence + ticket per workgroup): 74 us.)
constexpr int kSegOneBlock = 512, kSegOneWaves = kSegOneBlock / 64, kSegOneChunk = 256, kSegOneZ = 8;
constexpr int kSegOneOwn = kSegFusedMaxQ / kSegOneZ;      // interior vertices a workgroup can own (groups of 64 dealt round-robin)
#ifdef TUCH_SEG_CLOCKS
// diagnostic build only (tools/diag/seg_clocks.py): s_memrealtime (100 MHz) of every block at the phase boundaries of
// segment_one_kernel: [block][0] start, [1] interior vertices compacted, [2] caps, [3] entries walked, [4] end
__device__ unsigned long long g_seg_clocks[8192][8];
#define SEG_CLOCK(i) do { if (threadIdx.x == 0) { const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; if (blk < 8192) g_seg_clocks[blk][i] = __builtin_amdgcn_s_memrealtime(); } } while (0)
extern "C" int tuch_debug_seg_clocks(unsigned long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_seg_clocks), sizeof(unsigned long long) * 8192 * 8) == hipSuccess ? TUCH_OK : TUCH_ERR_HIP;
}
#else
#define SEG_CLOCK(i) do { } while (0)
#endif

__global__ __launch_bounds__(kSegOneBlock) void segment_one_kernel(
    const float* __restrict__ verts, const uint8_t* __restrict__ body_flags, uint8_t* __restrict__ exterior,
    const int32_t* __restrict__ seg_q_off, const int32_t* __restrict__ seg_q_vidx,
    const int32_t* __restrict__ cap_range, const int32_t* __restrict__ cap_off, const int32_t* __restrict__ cap_vidx,
    const int32_t* __restrict__ ent_off, const int32_t* __restrict__ ent,
    const int32_t* __restrict__ link_off, const int32_t* __restrict__ link, const int32_t* __restrict__ leaf_counts,
    const int32_t* __restrict__ vpos, int slots, int V, float thresh)
{
    __shared__ int32_t s_list[kSegFusedMaxQ];
    __shared__ int32_t s_cnt[kSegOneOwn];
    __shared__ float s_half[kSegOneOwn];
    __shared__ float sT[kSegOneChunk * 9];
    __shared__ float s_caps[kSegFusedMaxCaps * 3];
    __shared__ int32_t s_wave[kSegOneWaves];
    __shared__ int32_t s_n;
    const int sg = blockIdx.x, b = blockIdx.y, z = blockIdx.z, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* vb = verts + (size_t)b * V * 3;
    uint8_t* eb = exterior + (size_t)b * V;
    const int q_beg = seg_q_off[sg], nq = seg_q_off[sg + 1] - q_beg;
    SEG_CLOCK(0);
    // A.  All of a thread's flags are requested before the first is looked at (the rounds of the scan then only touch LDS).
    {
        const uint8_t* fb = body_flags + (size_t)b * V;
        constexpr int kRounds = kSegFusedMaxQ / kSegOneBlock;
        uint32_t interior = 0;                              // bit r: vertex r * block + t is interior
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int q = r * kSegOneBlock + t;
            if (q < nq && fb[seg_q_vidx[q_beg + q]] == 0) interior |= 1u << r;
        }
        if (t == 0) s_n = 0;
        __syncthreads();
        for (int r = 0; r * kSegOneBlock < nq; ++r) {
            const bool in = (interior >> r) & 1u;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(in);
            if (lane == 0) s_wave[wave] = __builtin_popcountll(bal);
            __syncthreads();
            int base = s_n;
            for (int w2 = 0; w2 < wave; ++w2) base += s_wave[w2];
            if (in) s_list[base + __builtin_popcountll(bal & ((1ull << lane) - 1ull))] = r * kSegOneBlock + t;
            __syncthreads();
            if (t == 0) { int add = 0; for (int w2 = 0; w2 < kSegOneWaves; ++w2) add += s_wave[w2]; s_n += add; }
            __syncthreads();
        }
    }
    const int n = s_n;
    const int groups = (n + 63) >> 6;
    const int mine = groups > z ? (groups - z + kSegOneZ - 1) / kSegOneZ : 0;      // own groups: z, z + Z, ...
    SEG_CLOCK(1);
    if (mine == 0) return;
    // B.
    const int c_lo = cap_range[sg];
    seg_fused_caps<kSegOneWaves>(vb, cap_off, cap_vidx, c_lo, cap_range[sg + 1], s_caps);
    SEG_CLOCK(2);
    // C.
    const P3 u_dir = {kFanX, kFanY, kFanZ};
    const P3 us = {shear_x(kFanX, kFanZ), shear_y(kFanY, kFanZ), kFanZ};
    const int e_beg = ent_off[sg], e_end = ent_off[sg + 1];
    const int slices = mine >= kSegOneWaves ? 1 : kSegOneWaves / mine;          // wavefronts per own group
    for (int j0 = 0; j0 < mine; j0 += kSegOneWaves) {                           // (one round unless n > 1024)
        const int j = slices > 1 ? wave / slices : j0 + wave;                    // own group, sub-slice of the entries
        const int sl = slices > 1 ? wave % slices : 0;
        const bool have = j < mine && (slices == 1 || wave < mine * slices);
        const int k = (z + (have ? j : 0) * kSegOneZ) * 64 + lane;               // position in the compacted list
        const int v0 = seg_q_vidx[q_beg + s_list[min(k, n - 1)]];
        const float qz = vb[3 * (size_t)v0 + 2];
        const float qx = shear_x(vb[3 * (size_t)v0], qz), qy = shear_y(vb[3 * (size_t)v0 + 1], qz);
        int crossings = 0;
        float half_sum = 0.0f;
        for (int chunk = e_beg; chunk < e_end; chunk += kSegOneChunk) {
            const int cn = min(kSegOneChunk, e_end - chunk);
            __syncthreads();
            for (int i = t; i < cn; i += kSegOneBlock) {
                const int id[3] = {ent[3 * (size_t)(chunk + i)], ent[3 * (size_t)(chunk + i) + 1], ent[3 * (size_t)(chunk + i) + 2]};
                float* dst = sT + i * 9;
                const int corners = id[2] < 0 ? 2 : 3;
                for (int c = 0; c < corners; ++c) {
                    const float* p = id[c] < V ? vb + 3 * (size_t)id[c] : s_caps + 3 * (id[c] - V - c_lo);
                    dst[3 * c] = shear_x(p[0], p[2]); dst[3 * c + 1] = shear_y(p[1], p[2]); dst[3 * c + 2] = p[2];
                }
                if (corners == 2) { dst[6] = (float)id[2]; dst[7] = kConeMarker; dst[8] = 0.0f; }
            }
            __syncthreads();
            if (!have) continue;
            for (int f = sl; f < cn; f += slices) {
                const float* e = sT + f * 9;
                if (e[7] != kConeMarker) {                              // a cap face (wave-uniform: LDS broadcast)
                    const P3 a = {e[0] - qx, e[1] - qy, e[2] - qz}, bb = {e[3] - qx, e[4] - qy, e[5] - qz}, c = {e[6] - qx, e[7] - qy, e[8] - qz};
                    const float ea = edge_fn(bb, c), eb2 = edge_fn(c, a), ec = edge_fn(a, bb);
                    const float numz = ea * a.z + eb2 * bb.z + ec * c.z;
                    const float mn = __builtin_fminf(__builtin_fminf(ea, eb2), ec), mx = __builtin_fmaxf(__builtin_fmaxf(ea, eb2), ec);
                    int n1 = (int)(__builtin_fminf(mn, numz) > 0.0f) - (int)(__builtin_fmaxf(mx, numz) < 0.0f);
                    const bool edge_zero = mn * mx == 0.0f;
                    if (__builtin_amdgcn_ballot_w64(edge_zero)) {
                        const bool tie = edge_zero & (numz != 0.0f);
                        if (__builtin_amdgcn_ballot_w64(tie)) {
                            if (tie) n1 = crossing_with_ties<true>(a, bb, c, ea, eb2, ec);
                        }
                    }
                    crossings += n1;
                } else {                                                // a boundary edge x -> y: the cone (u, x, y)
                    const P3 bb = {e[0] - qx, e[1] - qy, e[2] - qz}, c = {e[3] - qx, e[4] - qy, e[5] - qz};
                    const bool at_query = ((bb.x == 0.0f) & (bb.y == 0.0f) & (bb.z == 0.0f)) | ((c.x == 0.0f) & (c.y == 0.0f) & (c.z == 0.0f));
                    if (!at_query) {
                        const int mult = (int)e[6];
                        const P3 pb = {__builtin_fmaf(kShearX, bb.z, bb.x), __builtin_fmaf(kShearY, bb.z, bb.y), bb.z};
                        const P3 pc = {__builtin_fmaf(kShearX, c.z, c.x), __builtin_fmaf(kShearY, c.z, c.y), c.z};
                        int c1;
                        float h1;
                        cone_term(us, bb, c, u_dir, pb, pc, c1, h1);
                        crossings += mult * c1;
                        half_sum += (float)mult * h1;
                    }
                }
            }
        }
        // sums: [sub-slice][own group][lane] with several sub-slices (mine x slices <= 8 wavefronts), else [own group][lane]
        if (have) {
            const int at = slices > 1 ? (sl * mine + j) * 64 + lane : j * 64 + lane;
            s_cnt[at] = crossings;
            s_half[at] = half_sum;
        }
        if (slices > 1) break;
    }
    __syncthreads();
    SEG_CLOCK(3);
    // D. one thread per own interior vertex (all lanes of a wavefront stay: long link lists are shared out over it)
    auto pos = [&](int id, float (&o)[3]) {                // a vertex id of the segment tables (>= V: cap vertex)
        const float* p = id < V ? vb + 3 * (size_t)id : s_caps + 3 * (id - V - c_lo);
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    };
    for (int j = wave; j < mine; j += kSegOneWaves) {       // (wave-uniform)
        const int k = (z + j * kSegOneZ) * 64 + lane;
        const bool active = k < n;
        const int qq = q_beg + s_list[active ? k : 0];
        const int v = seg_q_vidx[qq];
        int cnt = 0;
        float half_sum = 0.0f;
        if (active) {
            if (slices > 1) {
                for (int s2 = 0; s2 < slices; ++s2) { cnt += s_cnt[(s2 * mine + j) * 64 + lane]; half_sum += s_half[(s2 * mine + j) * 64 + lane]; }
            } else {
                cnt = s_cnt[j * 64 + lane];
                half_sum = s_half[j * 64 + lane];
            }
            cnt += seg_leaf_count(leaf_counts + 2 * ((size_t)b * slots + vpos[v]), sg);
        }
        const float vx = vb[3 * (size_t)v], vy = vb[3 * (size_t)v + 1], vz = vb[3 * (size_t)v + 2];
        const float qx = shear_x(vx, vz), qy = shear_y(vy, vz);
        auto cone = [&](const float (&p0)[3], const float (&p1)[3], float ax, float ay, float az, float sx, float sy, float& h, int& c) {
            const P3 pb = {p0[0] - ax, p0[1] - ay, p0[2] - az}, pc = {p1[0] - ax, p1[1] - ay, p1[2] - az};
            const P3 sb = {shear_x(p0[0], p0[2]) - sx, shear_y(p0[1], p0[2]) - sy, p0[2] - az};
            const P3 sc = {shear_x(p1[0], p1[2]) - sx, shear_y(p1[1], p1[2]) - sy, p1[2] - az};
            int c1;
            float h1;
            cone_term(us, sb, sc, u_dir, pb, pc, c1, h1);
            h += h1;
            c += c1;
        };
        const int e0 = active ? link_off[qq] : 0, e1 = active ? link_off[qq + 1] : 0;
        constexpr int kLongLinks = 16;
        if (e1 - e0 <= kLongLinks) {
            for (int e = e0; e < e1; e += 2) {             // two links at a time: their four corners are fetched together
                int id[4];
                float pp[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u) id[u] = link[2 * min(e + (u >> 1), e1 - 1) + (u & 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) pos(id[u], pp[u]);
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (e + h < e1) cone(pp[2 * h], pp[2 * h + 1], vx, vy, vz, qx, qy, half_sum, cnt);
            }
        }
        unsigned long long todo = __builtin_amdgcn_ballot_w64(e1 - e0 > kLongLinks);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int le0 = __builtin_amdgcn_readlane(e0, src), le1 = __builtin_amdgcn_readlane(e1, src);
            const float lvx = __shfl(vx, src), lvy = __shfl(vy, src), lvz = __shfl(vz, src);
            const float lqx = __shfl(qx, src), lqy = __shfl(qy, src);
            float h = 0.0f;
            int cr = 0;
            for (int e = le0 + lane; e < le1; e += 64) {
                float a0[3], a1[3];
                pos(link[2 * e], a0);
                pos(link[2 * e + 1], a1);
                cone(a0, a1, lvx, lvy, lvz, lqx, lqy, h, cr);
            }
#pragma unroll
            for (int m2 = 32; m2 >= 1; m2 >>= 1) { h += __shfl_xor(h, m2); cr += __shfl_xor(cr, m2); }
            if (lane == src) { half_sum += h; cnt += cr; }
        }
        if (active) {
            const float w = (float)cnt - half_sum * (0.5f / kPi);
            if (!(w <= thresh)) eb[v] = 1;
        }
    }
    SEG_CLOCK(4);
}

}  // namespace

// can the segment filter run as the one launch above?  (flags only; the caller checks that)
bool tuch_ray_segment_fused_available(const tuch_contact_model* m)
{
    return m && m->seg_cap_off && m->seg_cap_range && m->seg_elem_mask && m->seg_q_max <= kSegFusedMaxQ && m->opt.seg_fused != 0;
}

// The segment filter as ONE launch (segment_one_kernel): kSegOneZ workgroups per (segment, body) read body_flags (the body
// test's own flags: a copy nobody writes during the call) and write ones into `exterior` [B,V]; leaf_counts =
// tuch_ray_segment_counts of the SAME vertices.
int tuch_ray_segment_flags_one(const tuch_contact_model* m, const float* verts, const uint8_t* body_flags,
                               const int32_t* leaf_counts, int B, float thresh, uint8_t* exterior, hipStream_t s)
{
    hipLaunchKernelGGL(segment_one_kernel, dim3(m->num_segments, B, kSegOneZ), dim3(kSegOneBlock), 0, s, verts, body_flags, exterior,
                       (const int32_t*)m->seg_q_off, (const int32_t*)m->seg_q_vidx, (const int32_t*)m->seg_cap_range,
                       (const int32_t*)m->cap_off, (const int32_t*)m->cap_vidx, (const int32_t*)m->seg_cap_off,
                       (const int32_t*)m->seg_cap_ent, (const int32_t*)m->seg_link_off, (const int32_t*)m->seg_link, leaf_counts,
                       (const int32_t*)m->seg_vpos, 2 * m->tree_qblocks * kRayQueries, m->V, thresh);
    return tuch_check_launch("tuch_ray_segment_flags_one");
}

bool tuch_ray_available(const tuch_contact_model* m)
{
    if (!m || m->tree_nodes <= 0 || !m->ring_off || m->tree_exact_len <= 0) return false;
    // ray_near_kernel's records hold the leaf in 16 bits (2 M faces; a mesh beyond that takes the solid-angle form)
    if (m->tree_leaves > 65535) return false;
    return m->opt.winding_ray != 0;
}

// room in the pair list, in (ray, leaf) pairs per query (a ray passes the slabs of ~4-5 leaves; option ray_pair_cap)
static int ray_pair_cap(const tuch_contact_model* m) { return m->opt.ray_pair_cap < 1 ? 1 : m->opt.ray_pair_cap; }

static RayLayout full_layout(const tuch_contact_model* m, int B, int Q, bool verts)
{
    RayLayout l;
    l.qblocks = verts ? 2 * m->tree_qblocks : ceil_div(Q, kRayQueries);
    // leaf strips are the first part of the tree stream; the caps behind them are never read
    l.T = ceil_div(m->tree_exact_len, 3) * 3 + 6;
    const int L = m->tree_leaves;
    const long cap = (long)ray_pair_cap(m) * Q;
    l.cap = (int)(cap < 0x3fffffffL ? cap : 0x3fffffffL);
    // tiles of a body, an upper bound: its pairs in 64s + one short tile per leaf (a leaf with fewer than 64 rays; a longer
    // leaf's remainder rides its last full tile); never fewer than the block-major fallback needs
    l.max_tiles = l.cap / 64 + L;
    if (l.max_tiles < l.qblocks * kFallbackChunks) l.max_tiles = l.qblocks * kFallbackChunks;
    // one column of wavefronts per XCD; twice what the chip holds at once (256 CUs x 4 SIMDs x 7 by registers), a
    // wavefront's share about two of the batch-64 step's ~35 k passes (TUCH_RAY_WAVES).  32 768 was chosen for ~51 k
    // tiles, one per wavefront; with a leaf's remainder riding its last full tile the step at batch 64 measured
    // 0.3692 / 0.3669 ms (16 384), 0.3703 / 0.3723 (24 576), 0.3746 / 0.3781 (32 768), two alternating runs each
    l.columns = B < 8 ? B : 8;
    const int waves = m->opt.ray_waves > 0 ? m->opt.ray_waves : 16384;
    l.workers = waves / l.columns > 0 ? waves / l.columns : 1;
    size_t o = 0;
    l.stream = tuch_ws_take(o, (size_t)B * l.T * sizeof(RayElem));
    l.bounds = tuch_ws_take(o, (size_t)B * m->tree_nodes * 2 * kSlabStride * sizeof(float));
    l.lists = tuch_ws_take(o, (size_t)B * l.qblocks * L * sizeof(RayEntry));
    l.list_len = tuch_ws_take(o, (size_t)B * l.qblocks * sizeof(int32_t));
    l.zeroed = o;                                                  // one memset: rays per leaf, fill cursors, crossing counts
    // (the span ray_stream_kernel clears in one go stays contiguous: no guards inside it, one behind it)
    l.leaf_cnt = tuch_ws_take(o, (size_t)B * L * sizeof(int32_t), false);
    l.leaf_fill = tuch_ws_take(o, (size_t)B * L * sizeof(int32_t), false);
    l.count = tuch_ws_take(o, (size_t)B * l.qblocks * kRayQueries * sizeof(int32_t), false);
    l.seg_count = o;
    if (verts && m->seg_elem_mask) o += align256(2 * (size_t)B * l.qblocks * kRayQueries * sizeof(int32_t));
    l.zeroed_bytes = o - l.zeroed;
    (void)tuch_ws_take(o, 0);
    l.leaf_off = tuch_ws_take(o, (size_t)B * L * sizeof(int32_t));
    l.tiles = tuch_ws_take(o, (size_t)B * l.max_tiles * sizeof(RayTile));
    l.body = tuch_ws_take(o, (size_t)B * sizeof(RayBody));
    l.pairs = tuch_ws_take(o, (size_t)B * l.cap * sizeof(int32_t));
    l.stats = tuch_ws_take(o, 256);
    l.boxes = tuch_ws_take(o, (size_t)B * l.T * sizeof(float4));     // the walk's filter box of every strip element
    l.total = o;
    return l;
}

void tuch_ray_layout_touch(const tuch_contact_model* m, int B, int Q)
{
    (void)full_layout(m, B, Q > 0 ? Q : m->V, Q <= 0);
}

size_t tuch_ray_workspace_bytes(const tuch_contact_model* m, int B, int Q)
{
    if (!m || m->tree_nodes <= 0 || B <= 0) return 0;
    const size_t a = full_layout(m, B, m->V, true).total;
    const size_t b = Q > 0 ? full_layout(m, B, Q, false).total : 0;
    return a > b ? a : b;
}

// sheared leaf strips and the slabs of every LEAF (inner nodes are not used by the flat near test)
static void launch_ray_boxes(const tuch_contact_model* m, const RayLayout& l, const float* verts, int B, char* ws, hipStream_t s,
                             bool one_launch, int keep_bounds = 0)
{
    RayElem* st = (RayElem*)(ws + l.stream);
    float* bounds = (float*)(ws + l.bounds);
    // one launch: every leaf poses its own run of the strip.  (Not for the points form with its far larger span of
    // counters to clear -- [B][Q] with Q = all HD points: the leaf grid has too few workgroups for that, 100 us)
    if (one_launch && m->tree_leaf_runs_tile) {
        hipLaunchKernelGGL(ray_leaf_bounds_kernel<true>, dim3(ceil_div(m->tree_leaves, kBoundsBlock / 16), B), dim3(kBoundsBlock), 0,
                           s, (const RayElem*)st, l.T, (const TreeNode*)m->tree_node, m->tree_nodes,
                           (const int32_t*)m->tree_height_off, (const int32_t*)m->tree_height_nodes, bounds, verts,
                           (const int32_t*)m->tree_vidx, (const float*)m->tree_sign_word, m->V, m->tree_exact_len, st,
                           (uint4*)(ws + l.zeroed), l.zeroed_bytes / sizeof(uint4), (float4*)(ws + l.boxes), keep_bounds);
        return;
    }
    hipLaunchKernelGGL(ray_stream_kernel, dim3(ceil_div(l.T, kBlock), B), dim3(kBlock), 0, s, verts,
                       (const int32_t*)m->tree_vidx, (const float*)m->tree_sign_word, m->V, m->tree_exact_len, l.T, st,
                       (uint4*)(ws + l.zeroed), l.zeroed_bytes / sizeof(uint4));
    hipLaunchKernelGGL(ray_leaf_bounds_kernel<false>, dim3(ceil_div(m->tree_leaves, kBoundsBlock / 16), B), dim3(kBoundsBlock), 0, s,
                       (const RayElem*)st, l.T, (const TreeNode*)m->tree_node, m->tree_nodes,
                       (const int32_t*)m->tree_height_off, (const int32_t*)m->tree_height_nodes, bounds,
                       (const float*)nullptr, (const int32_t*)nullptr, (const float*)nullptr, 0, m->tree_exact_len, (RayElem*)nullptr,
                       (uint4*)nullptr, (size_t)0, (float4*)(ws + l.boxes), keep_bounds);
}

// the near test.  waves = 0: four wavefronts per query block while the blocks alone do not fill the chip (see the kernel),
// one otherwise; 1 / 4: that form (tuch_ray_near_debug)
template <bool kVerts>
static void launch_ray_near(const tuch_contact_model* m, const RayLayout& l, const float* queries, const int32_t* counts, int B,
                            int Q, char* ws, hipStream_t s, unsigned long long* stats, float* rays_out, int waves)
{
    const int L = m->tree_leaves;
    const TreeNode* nodes = (const TreeNode*)m->tree_node;
    const int32_t* qperm = kVerts ? (const int32_t*)m->tree_qperm : nullptr;
    RayEntry* lists = (RayEntry*)(ws + l.lists);
    int32_t* list_len = (int32_t*)(ws + l.list_len);
    int32_t* leaf_cnt = (int32_t*)(ws + l.leaf_cnt);
    if (waves == 4 || (waves == 0 && (long)l.qblocks * B <= 2048))
        hipLaunchKernelGGL((ray_near_kernel<kVerts, 4>), dim3(l.qblocks, B), dim3(256), 0, s, queries, nodes,
                           (const float*)(ws + l.bounds), m->tree_nodes, L, qperm, counts, Q, l.qblocks, lists, list_len,
                           leaf_cnt, stats, rays_out);
    else
        hipLaunchKernelGGL((ray_near_kernel<kVerts, 1>), dim3(l.qblocks, B), dim3(64), 0, s, queries, nodes,
                           (const float*)(ws + l.bounds), m->tree_nodes, L, qperm, counts, Q, l.qblocks, lists, list_len,
                           leaf_cnt, stats, rays_out);
}

// near leaves -> rays per leaf -> tiles -> crossing counts (count[b][slot])
template <bool kVerts>
static int launch_ray_counts(const tuch_contact_model* m, const RayLayout& l, const float* verts, const float* queries,
                             const int32_t* counts, int B, int Q, char* ws, hipStream_t s, unsigned long long* stats)
{
    launch_ray_boxes(m, l, verts, B, ws, s, kVerts);  // clears the counters (l.zeroed) as well
    const int L = m->tree_leaves;
    const TreeNode* nodes = (const TreeNode*)m->tree_node;
    // the leaves are the height-0 entries of the tree's height table (tree_height_off_host[0] == 0)
    const int32_t* leaf_nodes = (const int32_t*)m->tree_height_nodes;
    const int32_t* qperm = kVerts ? (const int32_t*)m->tree_qperm : nullptr;
    RayEntry* lists = (RayEntry*)(ws + l.lists);
    int32_t* list_len = (int32_t*)(ws + l.list_len);
    int32_t* leaf_cnt = (int32_t*)(ws + l.leaf_cnt);
    int32_t* leaf_off = (int32_t*)(ws + l.leaf_off);
    RayTile* tiles = (RayTile*)(ws + l.tiles);
    RayBody* body = (RayBody*)(ws + l.body);
    int32_t* pairs = (int32_t*)(ws + l.pairs);
    launch_ray_near<kVerts>(m, l, queries, counts, B, Q, ws, s, stats, nullptr, 0);
    const size_t tf_lds = (2 * (size_t)L + l.qblocks + 1) * sizeof(int32_t);
    if (l.qblocks <= kFillMaxBlocks && tf_lds <= 48u * 1024)
        // (one-wave workgroups per body: 64, more for small batches -- the kernel is a chain of dependent steps per workgroup, and a
        // body's ~5000 list entries over 256 workgroups are one pass each: batch 8 0.180 -> 0.173 ms per step, batch 16 0.203 -> 0.199,
        // batch 32 / 64 unchanged / slower with more)
        hipLaunchKernelGGL(ray_tiles_fill_kernel, dim3(B, std::min(256, std::max(kFillSplit, 2048 / B))), dim3(kTilesFillBlock), tf_lds, s, (const int32_t*)leaf_cnt,
                           nodes, leaf_nodes, L, l.cap, l.max_tiles, l.qblocks * kFallbackChunks, tiles, body,
                           (const RayEntry*)lists, (const int32_t*)list_len, l.qblocks, (int32_t*)(ws + l.leaf_fill), pairs, L);
    else {
    hipLaunchKernelGGL(ray_tiles_kernel, dim3(B), dim3(kTilesBlock), 0, s, (const int32_t*)leaf_cnt, nodes, leaf_nodes, L, l.cap,
                       l.max_tiles, l.qblocks * kFallbackChunks, leaf_off, tiles, body);
    hipLaunchKernelGGL(ray_fill_kernel, dim3(l.qblocks, B), dim3(64), 0, s, (const RayEntry*)lists, (const int32_t*)list_len,
                       (const RayBody*)body, (const int32_t*)leaf_off, L, l.qblocks, l.cap, (int32_t*)(ws + l.leaf_fill), pairs);
    }
    const dim3 grid(l.columns, l.workers);
    const bool seg = kVerts && m->seg_elem_mask;
    const int32_t* vmask = (const int32_t*)m->seg_vmask;
    int32_t* seg_count = (int32_t*)(ws + l.seg_count);
#define TUCH_LAUNCH_RAY_LEAF(COUNT, SEG)                                                                                      \
    hipLaunchKernelGGL((ray_leaf_kernel<kVerts, COUNT, SEG>), grid, dim3(64), 0, s, queries, (const RayElem*)(ws + l.stream),  \
                       (const float4*)(ws + l.boxes), (const RayTile*)tiles, (const RayBody*)body, (const int32_t*)pairs, (const RayEntry*)lists,            \
                       (const int32_t*)list_len, nodes, L, qperm, counts, Q, l.T, l.qblocks, B, l.cap, l.max_tiles,           \
                       (int32_t*)(ws + l.count), stats, vmask, seg_count)
    if (stats) {
        if (seg) TUCH_LAUNCH_RAY_LEAF(true, kVerts); else TUCH_LAUNCH_RAY_LEAF(true, false);
    } else {
        if (seg) TUCH_LAUNCH_RAY_LEAF(false, kVerts); else TUCH_LAUNCH_RAY_LEAF(false, false);
    }
#undef TUCH_LAUNCH_RAY_LEAF
    return TUCH_OK;
}

int tuch_ray_exterior_verts(const tuch_contact_model* m, const float* verts, int B, float thresh, uint8_t* exterior,
                            float* w, void* workspace, hipStream_t s, unsigned long long* stats_host, uint8_t* exterior_copy)
{
    const RayLayout l = full_layout(m, B, m->V, true);
    char* ws = (char*)workspace;
    unsigned long long* stats = stats_host ? (unsigned long long*)(ws + l.stats) : nullptr;
    if (stats && hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), s) != hipSuccess) return TUCH_ERR_HIP;
    const int rc = launch_ray_counts<true>(m, l, verts, verts, nullptr, B, m->V, ws, s, stats);
    if (rc != TUCH_OK) return rc;
    if (w || exterior)
        hipLaunchKernelGGL(ray_finalize_verts_kernel, dim3(ceil_div(m->V, kBlock), B), dim3(kBlock), 0, s, verts,
                           (const int32_t*)(ws + l.count), (const int32_t*)m->tree_qperm, (const int32_t*)m->ring_off,
                           (const int32_t*)m->ring_vidx, m->V, l.qblocks * kRayQueries, thresh, w, exterior, exterior_copy);
    if (stats_host) {
        std::vector<RayBody> bodies((size_t)B);
        if (hipMemcpyAsync(stats_host, stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(bodies.data(), ws + l.body, (size_t)B * sizeof(RayBody), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return TUCH_ERR_HIP;
        unsigned long long tiles = 0;
        for (int b = 0; b < B; ++b) tiles += bodies[b].tiles;
        stats_host[3] = tiles;                     // passes of the crossing walk: the tiles of every body (counted, not extrapolated)
    }
    return tuch_check_launch("tuch_ray_exterior_verts");
}

const int32_t* tuch_ray_segment_counts(const tuch_contact_model* m, int B, const void* workspace)
{
    if (!m->seg_elem_mask) return nullptr;
    return (const int32_t*)((const char*)workspace + full_layout(m, B, m->V, true).seg_count);
}

int tuch_ray_exterior_points(const tuch_contact_model* m, const float* verts, const float* points, const int32_t* counts,
                             int B, int Q, float thresh, uint8_t* exterior, float* w, void* workspace, hipStream_t s)
{
    const RayLayout l = full_layout(m, B, Q, false);
    char* ws = (char*)workspace;
    const int rc = launch_ray_counts<false>(m, l, verts, points, counts, B, Q, ws, s, nullptr);
    if (rc != TUCH_OK) return rc;
    hipLaunchKernelGGL(ray_finalize_points_kernel, dim3(ceil_div(Q, kBlock), B), dim3(kBlock), 0, s,
                       (const int32_t*)(ws + l.count), counts, Q, l.qblocks * kRayQueries, thresh, w, exterior);
    return tuch_check_launch("tuch_ray_exterior_points");
}

// ---- tuch_ray_near_debug / tuch_near_encode_host: what the near lists hold, for the tests -------------------------------------
// bitmap [B][L][qblocks * 8]: bit (slot & 7) of byte (slot >> 3) is set where (leaf, slot) is listed (zeroed by the caller);
// leaves [B][qblocks][L]: the leaf of every entry of a block's list in list order, -1 behind its end
__global__ __launch_bounds__(64) void ray_near_bitmap_kernel(
    const RayEntry* __restrict__ lists, const int32_t* __restrict__ list_len, int L, int qblocks, uint8_t* __restrict__ bitmap,
    int32_t* __restrict__ leaves)
{
    const int qb = blockIdx.x, b = blockIdx.y;
    const size_t at = ((size_t)b * qblocks + qb) * L;
    const int n = min(list_len[(size_t)b * qblocks + qb], L);
    for (int j = threadIdx.x; j < L; j += 64) {
        const RayEntry e = j < n ? lists[at + j] : RayEntry{-1, 0, 0u, 0u};
        if (leaves) leaves[at + j] = e.leaf;
        if (bitmap && e.leaf >= 0 && e.leaf < L)
            *reinterpret_cast<uint2*>(bitmap + ((size_t)b * L + e.leaf) * ((size_t)qblocks * 8) + (size_t)qb * 8) = make_uint2(e.mask_lo, e.mask_hi);
    }
}

static int tuch_ray_near_debug_run(const tuch_contact_model* m, const float* verts, const float* points, const int32_t* counts,
                            int B, int Q, int waves, void* workspace, float* out_bounds, uint32_t* out_records,
                            float* out_rays, uint8_t* out_bitmap, int32_t* out_leaves, int32_t* out_len, hipStream_t s)
{
    const bool by_verts = points == nullptr;
    const RayLayout l = full_layout(m, B, by_verts ? m->V : Q, by_verts);
    char* ws = (char*)workspace;
    const int L = m->tree_leaves;
    launch_ray_boxes(m, l, verts, B, ws, s, by_verts, 1);
    if (by_verts) launch_ray_near<true>(m, l, verts, nullptr, B, m->V, ws, s, nullptr, out_rays, waves);
    else launch_ray_near<false>(m, l, points, counts, B, Q, ws, s, nullptr, out_rays, waves);
    const float* bounds = (const float*)(ws + l.bounds);
    if (out_bitmap && hipMemsetAsync(out_bitmap, 0, (size_t)B * L * l.qblocks * 8, s) != hipSuccess) return TUCH_ERR_HIP;
    hipLaunchKernelGGL(ray_near_bitmap_kernel, dim3(l.qblocks, B), dim3(64), 0, s, (const RayEntry*)(ws + l.lists),
                       (const int32_t*)(ws + l.list_len), L, l.qblocks, out_bitmap, out_leaves);
    if ((out_bounds && hipMemcpyAsync(out_bounds, bounds, (size_t)B * kNearSlabs * L * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (out_records && hipMemcpyAsync(out_records, bounds + near_records_at(B, L), (size_t)B * L * 8 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (out_len && hipMemcpyAsync(out_len, ws + l.list_len, (size_t)B * l.qblocks * sizeof(int32_t), hipMemcpyDeviceToDevice, s) != hipSuccess))
        return TUCH_ERR_HIP;
    return tuch_check_launch("tuch_ray_near_debug");
}

extern "C" int tuch_ray_near_debug(const tuch_contact_model* m, const float* verts, const float* points, const int32_t* counts,
                                   int B, int Q, int waves, void* workspace, size_t workspace_bytes, long long* dims_host,
                                   float* out_bounds, uint32_t* out_records, float* out_rays, uint8_t* out_bitmap,
                                   int32_t* out_leaves, int32_t* out_len, void* stream)
{
    TUCH_REQUIRE(m && dims_host, "tuch_ray_near_debug: null pointer");
    TUCH_REQUIRE(tuch_ray_available(m), "tuch_ray_near_debug: the model has no cluster tree / vertex rings");
    TUCH_REQUIRE(B > 0 && B <= 65535 && (!points || Q > 0), "tuch_ray_near_debug: bad sizes B=%d Q=%d", B, Q);
    TUCH_REQUIRE(waves == 0 || waves == 1 || waves == 4, "tuch_ray_near_debug: waves %d is not 0, 1 or 4", waves);
    dims_host[0] = m->tree_leaves;
    dims_host[1] = points ? ceil_div(Q, kRayQueries) : 2 * m->tree_qblocks;
    const size_t need = tuch_ray_workspace_bytes(m, B, points ? Q : 0);
    dims_host[2] = (long long)need;
    if (!verts) return TUCH_OK;                     // the sizes only
    if (!workspace || workspace_bytes < need) {
        tuch_set_error("tuch_ray_near_debug: workspace %zu < %zu bytes", workspace_bytes, need);
        return TUCH_ERR_WORKSPACE;
    }
    return tuch_ray_near_debug_run(m, verts, points, counts, B, Q, waves, workspace, out_bounds, out_records, out_rays,
                                   out_bitmap, out_leaves, out_len, (hipStream_t)stream);
}

extern "C" int tuch_near_encode_host(float value, int round_up, int* out)
{
    if (!out) return TUCH_ERR_ARG;
    *out = near_encode(value, round_up != 0);
    return TUCH_OK;
}

// The segment filter (winding.hip: caps, compacted interior vertices per (body, segment) in seg_count / seg_list) by
// ray crossings.  leaf_counts (tuch_ray_segment_counts of the SAME verts, or nullptr): the crossings with the body faces
// of the segments are taken from there and only cap faces and boundary edges are walked here.
// Scratch of the caller: seg_entries [B,seg_ray_total,9] floats filled by tuch_ray_segment_prepare (same `assisted`), seg_partial
// (two partial arrays + the work items).
// the part that needs only the vertices and the cap centroids (the caller runs it ahead of the body's inside test, off the
// critical chain): the posed, sheared entries.  assisted as in tuch_ray_segment_flags (leaf counts will be available).
void tuch_ray_segment_prepare(const tuch_contact_model* m, const float* verts, const float* caps, int assisted, int B,
                              float* seg_entries, hipStream_t s)
{
    const bool as = assisted && m->seg_cap_off;
    const int E = as ? m->seg_cap_total : m->seg_ray_total;
    hipLaunchKernelGGL(segment_shear_entries_kernel, dim3(ceil_div(E > 0 ? E : 1, kBlock), B), dim3(kBlock), 0, s,
                       verts, caps, (const int32_t*)(as ? m->seg_cap_ent : m->seg_ray_ent), m->V, m->num_caps, E, seg_entries);
}

int tuch_ray_segment_flags(const tuch_contact_model* m, const float* verts, const float* caps, const int32_t* seg_count,
                           const int32_t* seg_list, const int32_t* leaf_counts, int B, int nsplit, float thresh,
                           float* seg_entries, int32_t* seg_partial, float* seg_w, uint8_t* seg_ext, uint8_t* exterior,
                           hipStream_t s)
{
    const bool assisted = leaf_counts && m->seg_cap_off;
    const int E = assisted ? m->seg_cap_total : m->seg_ray_total;
    const int32_t* ent_off = (const int32_t*)(assisted ? m->seg_cap_off : m->seg_ray_off);
    float* partial_half = (float*)(seg_partial + (size_t)B * nsplit * m->seg_q_total);
    // work items behind the two partial arrays (B * num_seg_blocks int2 + 1 counter; the caller sizes seg_partial for it)
    int2* items = (int2*)(partial_half + (size_t)B * nsplit * m->seg_q_total);
    int32_t* items_total = (int32_t*)(items + (size_t)B * m->num_seg_blocks);
    const long worst = (long)B * m->num_seg_blocks * nsplit;
    const int grid = (int)(worst < 8192 ? worst : 8192);
    hipLaunchKernelGGL(segment_items_kernel, dim3(1), dim3(kItemsBlock), 0, s, seg_count, B * m->num_segments, items, items_total,
                       nsplit, grid);
    hipLaunchKernelGGL(segment_ray_kernel, dim3((unsigned)grid), dim3(64), 0, s, verts,
                       (const float*)seg_entries, (const int2*)items, (const int32_t*)items_total, (const int32_t*)m->seg_q_off,
                       (const int32_t*)m->seg_q_vidx, ent_off, seg_count, seg_list, m->V, E,
                       m->seg_q_total, m->num_segments, nsplit, seg_partial, partial_half);
    hipLaunchKernelGGL(segment_ray_finalize_kernel, dim3(ceil_div(m->seg_q_total, kBlock), B), dim3(kBlock), 0, s, verts, caps,
                       (const int32_t*)seg_partial, (const float*)partial_half, (const int32_t*)m->seg_of_q,
                       (const int32_t*)m->seg_q_off, (const int32_t*)m->seg_q_vidx, (const int32_t*)m->seg_link_off,
                       (const int32_t*)m->seg_link, seg_count, seg_list, assisted ? leaf_counts : nullptr,
                       (const int32_t*)m->seg_vpos, 2 * m->tree_qblocks * kRayQueries, m->V,
                       m->num_caps, m->seg_q_total, m->num_segments, nsplit, (const int32_t*)items_total, thresh, seg_w, seg_ext,
                       exterior);
    return tuch_check_launch("tuch_ray_segment_flags");
}
