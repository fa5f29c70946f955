// Closest point on the posed surface for arbitrary query points (tuch_closest_point, include/tuch_amd.h; tuch_cp_search
// for scan_fit.hip), its adjoint and the face groups it walks.
//
// Two launches:
//   cp_group_bounds_kernel  per (body, group): the posed corners of the group's faces, gathered in group order
//                           ([B][F][9] floats: what the search stages with coalesced loads), and their box ([B][G][8]:
//                           lo.xyz, -, hi.xyz, -)
//   cp_search_kernel        one query per lane, 64 consecutive queries of one body per wavefront (one wavefront per
//                           workgroup: staging is per wavefront, nothing is shared between wavefronts).  Sweep 1: the
//                           smallest farthest-corner distance over the body's boxes, an upper bound of the answer;
//                           the groups that give it to some lane (the seeds) are tested first, so that the walk starts
//                           from exact distances.  Sweep 2: a group is staged in LDS only when some lane's box lower
//                           bound is within its current best (ballot); the lanes whose own bound admits it run the
//                           exact test over its faces, every lane reading the same triangle (an LDS broadcast).  The
//                           next admitted group's loads are issued before the current group's tests (two LDS buffers).
// The adjoint (cp_bwd_kernel) scatters into the winning face's corner rows with fit_scatter_corners (fit_reduce.h: shared
// with scan_fit.hip's term) and converts fixed-point sums with tuch_launch_fixed_to_float (common.h).
//
// The rule.  cp_eval below is THE squared distance of a (query, triangle) pair: one instruction sequence (contraction
// off, every fused operation spelled out), a function of the six points' bits only.  The winner is the smallest packed
// key (d2 bits << 32 | face index): the smallest d2, among equal bits the smallest face.  Which groups are visited, in
// which order, by which lane or body never enters a key, so any conservative pruning gives the bits of the full sweep.
//
// Pruning margin.  With D^2 = far(g), the squared distance from the query to the farthest corner of group g's box
// (it bounds |p - a|, |p - b|, |p - c|, and |b - a|, |c - a| <= 2 D), the residual p - a - v (b - a) - w (c - a) is
// formed from terms of size <= 2 D with about a dozen roundings per component: its error is below 21 u D
// (u = 2^-24), the error of its squared length below 45 u D^2, and the two box distances carry 4 u each.  The
// returned point lies in the triangle (v, w are clamped), hence in the box.  So for every face f of g
//     lb(g) - 64 u far(g)  <=  computed d2(f)  <=  far(g) (1 + 64 u),
// and a group is skipped for a lane only when lb(g) - 64 u far(g) is GREATER than the lane's bound (the best computed
// d2 so far, at the start min_g far(g) (1 + 64 u)): no face of it can produce a key that is smaller or equal.
//
// The hinted start (tuch_closest_point with a hint).  hint [B,Q] names, per query, a face that is probably the answer -- in
// a fitting loop the previous iteration's.  The hint is only a bound: a lane whose hint is a face index in [0, F)
// (checked before it addresses anything) runs cp_eval on that face's posed corners and enters the result as an
// ordinary key; its bound starts at that exact d2, its seed is the face's group (cp_face_group, the inverse of
// cp_face_list), and it takes no part in sweep 1, which is skipped when no lane of the wavefront needs it.  The key is
// a computed key of a face, one the full sweep computes too, so it cannot undercut the full sweep's minimum, and
// lb(g) - 64 u far(g) <= bound still admits every group that can hold a smaller or equal key: a face with a smaller
// d2, or with equal bits and a smaller index, has computed d2 <= bound and by the inequality above makes its group's
// lb - 64 u far <= bound.  A lane whose hint is out of range, or whose hinted d2 is not finite (a NaN bound would
// compare false with everything and admit nothing), takes the unhinted path.  So the outputs equal the unhinted
// call's bit for bit for every content of hint.  hint may alias the face output: a lane reads only its own entry, and
// before it writes its face (a wholly padded block writes without reading).
//
// The oriented search (tuch_closest_point with normals; cp_search_kernel<*, true>, cp_group_bounds_kernel<true>).  A query
// is (p, n).  cp_admissible below is THE admissibility of a (normal, triangle) pair, stated in include/tuch_amd.h: with
// m = (b - a) x (c - a), mm = |m|^2, nn = |n|^2, s = m . n, every operation rounded to float32 on its own,
//     admissible  <=>  s > 0  and  s s >= c2 (mm nn),      c2 = c c,  c = (float)cos(max_angle).
// It is a function of the pair's bits and c only, so the admissible set of a query never depends on group, lane, batch
// or order, and the winner -- the smallest key over that set, cp_eval untouched -- is the unpruned sweep's whatever is
// pruned conservatively.  A lane whose nn is 0 or not finite is unconstrained: cp_admissible is not asked, and all
// that follows treats every group as wholly admissible for it, which is the unoriented search.
//   The upper bound.  "min_g far(g) (1 + 64 u)" bounds the answer only if group g holds a face the lane may take.  A
// constrained lane therefore starts its bound from (a) the exact d2 of its hint, if that face is admissible for it,
// or (b) far(g) (1 + 64 u) of a group that is WHOLLY ADMISSIBLE for it: not empty, every slot a face, every face
// admissible (then the inequality of the pruning margin holds for an admissible face of g), or (c) +inf.  Under a bound
// of +inf every group whose lb is finite is admitted until an admissible face has been found; the first group a lane
// tests (its seed) is then the nearest group, by far(g), that is not wholly inadmissible.  A seed is only a group
// tested first: it carries no bound.
//   The cones.  cp_group_bounds_kernel<true> stores per (body, group) an axis A (the normalised sum of the faces' unit
// normals m / |m|), cos beta and sin beta of the largest angle beta between A and one of them, the smallest and the
// largest mm, and a flag: usable only if every slot of the group is a face with kCpSaneLo <= mm <= kCpSaneHi and the
// sum has a direction.  Nothing in it depends on the queries.  With alpha the angle between A and n, every face normal
// of the group makes an angle in [alpha - beta, alpha + beta] with n, so for a lane with kCpNormalLo <= nn <= kCpNormalHi,
// kCpPairLo <= mm nn <= kCpPairHi for every face of the group, and max_angle = theta <= 90 deg:
//     wholly admissible    if  cos alpha > 0, cos beta > 0 and cos(alpha + beta) >= c + kCpConeMargin
//                          (alpha, beta < 90 deg, so alpha + beta < 180 deg where the cosine is monotone:
//                          alpha + beta < theta, every face is within theta of n);
//     wholly inadmissible  if  cos alpha < cos beta - kCpConeMargin (alpha > beta: the cone does not hold n) and
//                          cos(alpha - beta) <= c - kCpConeMargin (0 < alpha - beta <= 180 deg, monotone again:
//                          alpha - beta > theta, no face is within theta of n);
//     mixed otherwise, and always for an unusable cone or a lane outside the sane range: the rule decides per face.
// cos(alpha +- beta) = cos alpha cos beta -+ sin alpha sin beta, with sin alpha = |A x n| / |n| and sin beta = |A x m^|
// of the face that attains beta: cross products, not sqrt(1 - cos^2), which loses half the digits near 0.
//   The margin.  With mm nn in [1e-24, 1e24] nothing in the rule overflows, and what underflows is harmless: s s and
// c2 (mm nn) are compared with an absolute error of one denormal step, 1.4e-45, that is 1.4e-21 relative to mm nn,
// which moves the cosine the comparison decides on by less than sqrt(1.4e-21) = 4e-11.  (The lane's own range,
// kCpNormalLo <= nn <= kCpNormalHi, is narrower than the faces': |A x n|^2 is formed before the division by |n| and
// must neither overflow nor lose a sine above 1e-9 to underflow.)  So with u = 2^-24: s carries an absolute error
// below 3 u |m| |n|, mm nn and c2 (mm nn) and s s a relative one below 7 u together, and the computed rule decides
// "cos angle(m, n) >= c" for the m it
// computed with the threshold moved by less than 8 u.  A, m^ and n / |n| are unit vectors to 3 u each; a dot or cross
// product of two of them adds 3 u; so each of cos alpha, sin alpha, cos beta, sin beta is within 10 u, a product of two
// of them within 21 u, cos(alpha +- beta) within 43 u, and with the rule's 8 u the two sides of either comparison
// differ from the exact ones by less than 51 u.  kCpConeMargin = 256 u is five times that: a misclassification can
// only go towards "mixed", which costs time and no bit.  (A wrong "wholly admissible" would make the bound invalid, a
// wrong "wholly inadmissible" would drop the winner: tests/test_gpu_oriented_point.py regroups the faces to catch
// either.)  The cones are computed from the m the rule computes, so a thin face whose computed m is far from its true
// normal is classified by what the rule will see.
//   How the sweeps use it.  Sweep 1 takes bound and seed from wholly admissible groups (and the nearest mixed group as
// the seed where it is nearer); a wholly inadmissible group is never tested by the lane -- cp_next_group gives it a
// NaN lower bound, which no bound admits -- and a group no lane admits is not staged.  Mixed groups are admitted by the
// box bound alone; in the exact test cp_eval runs only for the faces cp_admissible passes (a branch: where a wavefront's
// queries face the same way, whole faces are skipped by all 64 lanes).  m is recomputed from the staged corners by the
// lane, by the same sequence the cone kernel and the hinted start use.
//   The hint.  A hinted lane starts from its hint only if the face is in [0, F), admissible for the lane and at a finite
// d2; then its key is one the unpruned sweep computes too, and the argument of the hinted start holds.  Any other hint
// takes the unhinted path.
#include "face_normal.h"
#include "fit_reduce.h"
#include "model.h"
#include "workspace.h"

namespace {

constexpr int kCpGroupFaces = 64;                   // most faces in a group (model.hip: build_closest_point_tables)
constexpr int kCpTri = 9;                           // floats per staged triangle
constexpr int kCpBox = 8;                           // floats per box
constexpr float kCpMargin = 64.0f * 5.9604645e-8f;  // 64 * 2^-24, relative to far(g)
constexpr float kCpDegenerate = 1e-8f;              // |ab x ac|^2 <= this * |ab|^2 |ac|^2: the triangle is its edges
// (kCpCone, kCpConeMargin and the sane ranges kCpSane*, kCpNormal*, kCpPair* of the cones: face_normal.h)
constexpr unsigned long long kCpNoKey = 0x7f800000ffffffffull;     // d2 = +inf, face = -1

struct CpLayout { size_t boxes, tris, cones, total; };

// oriented: the unoriented layout, then the cones
CpLayout cp_layout(const tuch_contact_model* m, int B, bool oriented)
{
    CpLayout l;
    size_t o = 0;
    l.boxes = tuch_ws_take(o, (size_t)B * m->cp_groups * kCpBox * sizeof(float));
    l.tris = tuch_ws_take(o, (size_t)B * m->F * kCpTri * sizeof(float));
    l.cones = oriented ? tuch_ws_take(o, (size_t)B * m->cp_groups * kCpCone * sizeof(float)) : o;
    l.total = o;
    return l;
}

static __device__ __forceinline__ int cp_clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

#pragma clang fp contract(off)
static __device__ __forceinline__ float cp_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

// n / d, 0 where d is not positive (a degenerate edge or triangle: the clamp below then picks an end point)
static __device__ __forceinline__ float cp_ratio(float n, float d) { return d > 0.0f ? n / d : 0.0f; }
static __device__ __forceinline__ float cp_clamp(float x, float hi) { return __builtin_fminf(__builtin_fmaxf(x, 0.0f), hi); }

// nearest point of the segment o + t e, t in [0, 1], to the point o + r: t and the squared distance
static __device__ __forceinline__ float cp_segment(float ex, float ey, float ez, float rx, float ry, float rz, float& t)
{
    t = cp_clamp(cp_ratio(cp_dot(ex, ey, ez, rx, ry, rz), cp_dot(ex, ey, ez, ex, ey, ez)), 1.0f);
    const float x = rx - t * ex, y = ry - t * ey, z = rz - t * ez;
    return cp_dot(x, y, z, x, y, z);
}

// Squared distance from p to the triangle (a, b, c) and the weights of the nearest point a + v (b - a) + w (c - a).
// The seven-region construction (the three corners, the three edges, the interior, told apart by the signs of eight dot
// products and three edge functions), every quotient guarded and v, w clamped into the triangle: whatever rounding
// does to the classification, the point is a point of the triangle.  A triangle without area (coincident or collinear
// corners) is the union of its edges: the nearest of the three segment answers, the first on ties.  So is, to float32,
// one thinner than 1e-4 of its edges (sin^2 of the angle at a <= kCpDegenerate): the nearest edge point is within half
// its height h of the nearest point in the plane, the squared distances differ by at most h^2 / 4 <= 2.5e-9 edge^2.
static __device__ __forceinline__ float cp_eval(float px, float py, float pz, const float* __restrict__ t, float& v, float& w)
{
    const float abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
    const float acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
    const float apx = px - t[0], apy = py - t[1], apz = pz - t[2];
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float nn = cp_dot(nx, ny, nz, nx, ny, nz);
    const float ll = cp_dot(abx, aby, abz, abx, aby, abz) * cp_dot(acx, acy, acz, acx, acy, acz);
    const float bpx = px - t[3], bpy = py - t[4], bpz = pz - t[5];
    if (!(nn > kCpDegenerate * ll)) {
        float tab, tac, tbc;
        const float dab = cp_segment(abx, aby, abz, apx, apy, apz, tab);
        const float dac = cp_segment(acx, acy, acz, apx, apy, apz, tac);
        const float dbc = cp_segment(t[6] - t[3], t[7] - t[4], t[8] - t[5], bpx, bpy, bpz, tbc);
        float d = dab;
        v = tab;
        w = 0.0f;
        if (dac < d) { d = dac; v = 0.0f; w = tac; }
        if (dbc < d) { d = dbc; v = 1.0f - tbc; w = tbc; }
        return d;
    }
    const float cpx = px - t[6], cpy = py - t[7], cpz = pz - t[8];
    const float bcx = t[6] - t[3], bcy = t[7] - t[4], bcz = t[8] - t[5];
    const float d1 = cp_dot(abx, aby, abz, apx, apy, apz), d2 = cp_dot(acx, acy, acz, apx, apy, apz);
    const float d3 = cp_dot(abx, aby, abz, bpx, bpy, bpz), d4 = cp_dot(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = cp_dot(abx, aby, abz, cpx, cpy, cpz), d6 = cp_dot(acx, acy, acz, cpx, cpy, cpz);
    const float eb = cp_dot(bcx, bcy, bcz, bpx, bpy, bpz), ec = -cp_dot(bcx, bcy, bcz, cpx, cpy, cpz);
    // on which side of each edge the projection falls: n . (edge x (p - its first corner)), products of an edge with a
    // point difference (no product of two point differences: a far query would drown the sign in its own square)
    const float vc = cp_dot(nx, ny, nz, aby * apz - abz * apy, abz * apx - abx * apz, abx * apy - aby * apx);
    const float va = cp_dot(nx, ny, nz, bcy * bpz - bcz * bpy, bcz * bpx - bcx * bpz, bcx * bpy - bcy * bpx);
    const float vb = cp_dot(nx, ny, nz, cpy * acz - cpz * acy, cpz * acx - cpx * acz, cpx * acy - cpy * acx);
    // one quotient: (numerator, denominator) by region; the interior takes 1 / |n|^2 (= va + vb + vc, without their noise)
    float num = 1.0f, den = nn;
    int region = 6;
    if (va <= 0.0f && eb >= 0.0f && ec >= 0.0f) { region = 5; num = eb; den = eb + ec; }            // edge bc
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { region = 4; num = d2; den = d2 - d6; }            // edge ac
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { region = 3; num = d1; den = d1 - d3; }            // edge ab
    if (d6 >= 0.0f && d5 <= d6) region = 2;                                                          // corner c
    if (d3 >= 0.0f && d4 <= d3) region = 1;                                                          // corner b
    if (d1 <= 0.0f && d2 <= 0.0f) region = 0;                                                        // corner a
    const float q = cp_ratio(num, den);
    v = region == 6 ? vb * q : region == 5 ? 1.0f - q : region == 3 ? q : region == 1 ? 1.0f : 0.0f;
    w = region == 6 ? vc * q : (region == 5 || region == 4) ? q : region == 2 ? 1.0f : 0.0f;
    v = cp_clamp(v, 1.0f);
    w = cp_clamp(w, 1.0f - v);
    const float x = (apx - v * abx) - w * acx, y = (apy - v * aby) - w * acy, z = (apz - v * abz) - w * acz;
    return cp_dot(x, y, z, x, y, z);
}

// squared distances from p to the box's nearest point (0 inside) and to its farthest corner
static __device__ __forceinline__ void cp_box(float px, float py, float pz, const float* __restrict__ box, float& lb, float& far)
{
    const float lx = box[0] - px, ly = box[1] - py, lz = box[2] - pz;
    const float hx = px - box[4], hy = py - box[5], hz = pz - box[6];
    const float nx = __builtin_fmaxf(__builtin_fmaxf(lx, hx), 0.0f), ny = __builtin_fmaxf(__builtin_fmaxf(ly, hy), 0.0f),
                nz = __builtin_fmaxf(__builtin_fmaxf(lz, hz), 0.0f);
    const float fx = __builtin_fmaxf(-lx, -hx), fy = __builtin_fmaxf(-ly, -hy), fz = __builtin_fmaxf(-lz, -hz);
    lb = cp_dot(nx, ny, nz, nx, ny, nz);
    far = cp_dot(fx, fy, fz, fx, fy, fz);
}

// (cp_face_normal, the face normal of the admissibility rule, is in face_normal.h: the vertex normals sum it too)

static __device__ __forceinline__ float cp_sq3(float x, float y, float z) { return (x * x + y * y) + z * z; }

// THE admissibility of a (query normal, triangle) pair (file header: the oriented search): s > 0 and s^2 >= c2 (mm nn),
// one sequence wherever it runs; false for a face without area (s = 0) and for NaN corners
static __device__ __forceinline__ bool cp_admissible(const float* __restrict__ t, float nx, float ny, float nz, float nn, float c2)
{
    float mx, my, mz;
    cp_face_normal(t, mx, my, mz);
    const float mm = cp_sq3(mx, my, mz);
    const float s = (mx * nx + my * ny) + mz * nz;
    return s > 0.0f && s * s >= c2 * (mm * nn);
}
#pragma clang fp contract(fast)

// (cp_cone_class, a cone against one lane's normal, is in face_normal.h with its constants: the point cloud's block
// cones are classified by the same function)

// what a lane of the oriented search knows of its normal: n and nn as the rule takes them, 1 / |n| for the cones
struct CpNormal {
    float x, y, z, nn;          // the rule's operands
    float inv;                  // 1 / |n| (cones only; 0 where they may not classify)
    bool constrained;           // nn is positive and finite: the rule applies (otherwise every face is admissible)
    bool conable;               // nn in [kCpNormalLo, kCpNormalHi]: the cones may classify for this lane
};

// the class of group g for a lane: an unconstrained lane admits everything, a constrained lane outside the sane range
// leaves every group to the exact rule
static __device__ __forceinline__ int cp_lane_class(const CpNormal& nm, const float* __restrict__ cones, int g, float c)
{
    if (!nm.constrained) return 1;
    if (!nm.conable) return 0;
    return cp_cone_class(cones + (size_t)g * kCpCone, nm.x, nm.y, nm.z, nm.inv, c);
}

template <bool kCone>
__global__ __launch_bounds__(64) void cp_group_bounds_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ face_list,
                                                            const int32_t* __restrict__ group_off, int V, int F, int G,
                                                            float* __restrict__ boxes, float* __restrict__ tris,
                                                            float* __restrict__ cones)
{
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int first = group_off[g];
    int n = group_off[g + 1] - first;
    n = n > kCpGroupFaces ? kCpGroupFaces : n;
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    const int slot = first + lane;
    const bool has_face = lane < n && slot >= 0 && slot < F;
    float t[kCpTri] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (has_face) {
        const int f = cp_clamp_index(face_list[slot], F);
        float* out = tris + ((size_t)b * F + slot) * kCpTri;
        for (int k = 0; k < 3; ++k) {
            const int vi = cp_clamp_index(faces[(size_t)f * 3 + k], V);
            const float* x = verts + ((size_t)b * V + vi) * 3;
            for (int c = 0; c < 3; ++c) {
                out[3 * k + c] = x[c];
                if (kCone) t[3 * k + c] = x[c];
                lo[c] = __builtin_fminf(lo[c], x[c]);
                hi[c] = __builtin_fmaxf(hi[c], x[c]);
            }
        }
    }
    if (kCone) {
        // The group's normal cone (file header): the axis is the normalised sum of the unit face normals, beta the
        // largest angle between the axis and one of them, kept as the (cos, sin) of the face that attains it.  Usable
        // only when every slot of the group is a face whose |m|^2 is in the sane range and the sum has a direction.
        float mx, my, mz;
        cp_face_normal(t, mx, my, mz);
        const float mm = cp_sq3(mx, my, mz);
        const bool sane = has_face && mm >= kCpSaneLo && mm <= kCpSaneHi;
        const float inv = sane ? 1.0f / __builtin_sqrtf(mm) : 0.0f;
        const float ux = mx * inv, uy = my * inv, uz = mz * inv;
        float sx = ux, sy = uy, sz = uz;
        for (int d = 32; d > 0; d >>= 1) {
            sx += __shfl_xor(sx, d, 64);
            sy += __shfl_xor(sy, d, 64);
            sz += __shfl_xor(sz, d, 64);
        }
        sx = __shfl(sx, 0, 64); sy = __shfl(sy, 0, 64); sz = __shfl(sz, 0, 64);
        const float len2 = sx * sx + sy * sy + sz * sz;
        const bool usable = n > 0 && __popcll(__ballot(sane)) == n && len2 >= 1e-6f && len2 <= 1e8f;
        const float il = usable ? 1.0f / __builtin_sqrtf(len2) : 0.0f;
        const float ax = sx * il, ay = sy * il, az = sz * il;
        const float wx = ay * uz - az * uy, wy = az * ux - ax * uz, wz = ax * uy - ay * ux;
        const float ca = sane ? ax * ux + ay * uy + az * uz : 2.0f;
        const float sa = __builtin_sqrtf(wx * wx + wy * wy + wz * wz);
        float cb = ca;
        for (int d = 32; d > 0; d >>= 1) cb = __builtin_fminf(cb, __shfl_xor(cb, d, 64));
        cb = __shfl(cb, 0, 64);
        const unsigned long long who = __ballot(ca == cb);
        const float sb = __shfl(sa, who ? __ffsll((long long)who) - 1 : 0, 64);
        float mm_lo = sane ? mm : inf, mm_hi = sane ? mm : 0.0f;
        for (int d = 32; d > 0; d >>= 1) {
            mm_lo = __builtin_fminf(mm_lo, __shfl_xor(mm_lo, d, 64));
            mm_hi = __builtin_fmaxf(mm_hi, __shfl_xor(mm_hi, d, 64));
        }
        if (lane == 0) {
            float* cone = cones + ((size_t)b * G + g) * kCpCone;
            cone[0] = ax; cone[1] = ay; cone[2] = az; cone[3] = cb;
            cone[4] = sb; cone[5] = usable && who ? 1.0f : 0.0f; cone[6] = mm_lo; cone[7] = mm_hi;
        }
    }
    for (int d = 32; d > 0; d >>= 1)
        for (int c = 0; c < 3; ++c) {
            lo[c] = __builtin_fminf(lo[c], __shfl_xor(lo[c], d, 64));
            hi[c] = __builtin_fmaxf(hi[c], __shfl_xor(hi[c], d, 64));
        }
    if (lane == 0) {
        float* box = boxes + ((size_t)b * G + g) * kCpBox;
        box[0] = lo[0]; box[1] = lo[1]; box[2] = lo[2]; box[3] = 0.0f;
        box[4] = hi[0]; box[5] = hi[1]; box[6] = hi[2]; box[7] = 0.0f;
    }
}

// the first group at or behind g that some lane admits (G: none) and that was not visited as a seed; lbm = this lane's
// lb - margin * far of that group.  kOriented: NaN (admitted under no bound) where the group's cone shows that no face
// of it is admissible for this lane.
template <bool kOriented>
static __device__ __forceinline__ int cp_next_group(const float* __restrict__ box, int G, int g, float px, float py, float pz,
                                                    float bound, bool active, int seed, float& lbm, const CpNormal& nm,
                                                    const float* __restrict__ cones, float c)
{
    for (; g < G; ++g) {
        float lb, far;
        cp_box(px, py, pz, box + (size_t)g * kCpBox, lb, far);
        lbm = lb - kCpMargin * far;
        if (kOriented && cp_lane_class(nm, cones, g, c) == 2) lbm = __builtin_nanf("");
        if (__ballot(active && seed == g) == 0ull && __ballot(active && lbm <= bound) != 0ull) break;
    }
    return g;
}

struct CpStage { float x[kCpTri]; int32_t fid; };

// this lane's share of a group: floats lane, lane + 64, ... of its 9 n contiguous floats, and the face of slot `lane`
static __device__ __forceinline__ void cp_stage_load(CpStage& r, const float* __restrict__ tris, const int32_t* __restrict__ face_list,
                                                     int first, int n, int lane)
{
    for (int k = 0; k < kCpTri; ++k) {
        const int i = lane + 64 * k;
        r.x[k] = i < n * kCpTri ? tris[(size_t)first * kCpTri + i] : 0.0f;
    }
    r.fid = lane < n ? face_list[first + lane] : -1;
}

static __device__ __forceinline__ void cp_stage_store(float* __restrict__ s_tri, int32_t* __restrict__ s_fid, const CpStage& r, int n,
                                                      int lane)
{
    for (int k = 0; k < kCpTri; ++k) {
        const int i = lane + 64 * k;
        if (i < n * kCpTri) s_tri[i] = r.x[k];
    }
    if (lane < n) s_fid[lane] = r.fid;
}

// faces [first, first + n) of group g, n = 0 for a range that does not lie in the face list
static __device__ __forceinline__ void cp_group_range(const int32_t* __restrict__ group_off, int g, int F, int& first, int& n)
{
    first = group_off[g];
    n = group_off[g + 1] - first;
    n = n > kCpGroupFaces ? kCpGroupFaces : (n < 0 ? 0 : n);
    if (first < 0 || first + n > F) n = 0;
}

// the exact test of one lane over a staged group: the smallest key (kOriented: over the faces admissible for the lane)
template <bool kOriented>
static __device__ __forceinline__ unsigned long long cp_test_group(float px, float py, float pz, const float* s_tri, const int32_t* s_fid,
                                                                   int n, unsigned long long key, const CpNormal& nm, float c2)
{
    for (int i = 0; i < n; ++i) {
        if (kOriented && nm.constrained && !cp_admissible(s_tri + i * kCpTri, nm.x, nm.y, nm.z, nm.nn, c2)) continue;
        float v, w;
        const float d = cp_eval(px, py, pz, s_tri + i * kCpTri, v, w);
        const unsigned long long k2 = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)s_fid[i];
        key = k2 < key ? k2 : key;
    }
    return key;
}

// the posed corners of face f (in [0, F)) of one body, as cp_eval takes them
static __device__ __forceinline__ void cp_face_corners(const int32_t* __restrict__ faces, const float* __restrict__ body_verts, int V,
                                                       int f, float* t)
{
    for (int k = 0; k < 3; ++k) {
        const int vi = cp_clamp_index(faces[(size_t)f * 3 + k], V);
        const float* x = body_verts + (size_t)vi * 3;
        t[3 * k] = x[0]; t[3 * k + 1] = x[1]; t[3 * k + 2] = x[2];
    }
}

// kHinted: hint [B,Q] is read (file header: the hinted start); hint and out_face may be the same memory, so neither is
// __restrict__.  Without it the kernel is the unhinted search, instruction for instruction.
// shift [B,3] or nullptr: the query is points - shift[b], one float32 subtraction per component (scan_fit.hip: the
// scan in the frame of the untranslated mesh); p - 0 has p's bits.
// kOriented: normals [B,Q,3] and cones [B,G,8] are read, c = cos(max_angle) and c2 = c * c as the host rounded them (file
// header: the oriented search).  Without it none of the four is touched.
template <bool kHinted, bool kOriented>
__global__ __launch_bounds__(64) void cp_search_kernel(const float* __restrict__ points, const float* __restrict__ shift,
                                                      const int32_t* __restrict__ counts, const int32_t* hint, const int32_t* __restrict__ face_group,
                                                      const float* __restrict__ boxes, const float* __restrict__ tris,
                                                      const int32_t* __restrict__ group_off, const int32_t* __restrict__ face_list,
                                                      const int32_t* __restrict__ faces, const float* __restrict__ verts,
                                                      int V, int F, int G, int Q, float* __restrict__ out_d2,
                                                      int32_t* out_face, float* __restrict__ out_bary,
                                                      const float* __restrict__ normals, const float* __restrict__ all_cones,
                                                      float c, float c2)
{
    __shared__ float s_tri[2][kCpGroupFaces * kCpTri];
    __shared__ int32_t s_fid[2][kCpGroupFaces];
    const int lane = threadIdx.x, b = blockIdx.y;
    const int q = blockIdx.x * 64 + lane;
    int count = Q;
    if (counts) {
        count = counts[b];
        count = count < 0 ? 0 : (count > Q ? Q : count);
    }
    if (blockIdx.x * 64 >= count) {       // a wholly padded block (wave-uniform)
        if (q < Q) {
            const size_t o = (size_t)b * Q + q;
            out_d2[o] = __builtin_huge_valf();
            out_face[o] = -1;
            out_bary[o * 3] = out_bary[o * 3 + 1] = out_bary[o * 3 + 2] = 0.0f;
        }
        return;
    }
    const bool active = q < count;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (active) {
        const float* p = points + ((size_t)b * Q + q) * 3;
        px = p[0]; py = p[1]; pz = p[2];
        if (shift) { px -= shift[3 * b]; py -= shift[3 * b + 1]; pz -= shift[3 * b + 2]; }
    }
    const float* box = boxes + (size_t)b * G * kCpBox;
    const float* body_tris = tris + (size_t)b * F * kCpTri;
    CpNormal nm = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, false, false};
    const float* cones = nullptr;
    if (kOriented) {
        cones = all_cones + (size_t)b * G * kCpCone;
        if (active) {
            const float* nq = normals + ((size_t)b * Q + q) * 3;
            nm.x = nq[0]; nm.y = nq[1]; nm.z = nq[2];
            nm.nn = cp_sq3(nm.x, nm.y, nm.z);
            nm.constrained = nm.nn > 0.0f && nm.nn < __builtin_huge_valf();
            nm.conable = nm.nn >= kCpNormalLo && nm.nn <= kCpNormalHi;
            nm.inv = nm.conable ? 1.0f / __builtin_sqrtf(nm.nn) : 0.0f;
        }
    }
    // the hinted start: the hinted face's own key, its exact d2 as the bound, its group as the seed
    unsigned long long key = kCpNoKey;
    bool hinted = false;
    int seed = -1;
    if (kHinted && active) {
        const int h = hint[(size_t)b * Q + q];
        if (h >= 0 && h < F) {
            const int hg = face_group[h];
            float t[kCpTri], v, w;
            cp_face_corners(faces, verts + (size_t)b * V * 3, V, h, t);
            const float d = cp_eval(px, py, pz, t, v, w);
            // (false for a NaN d: that lane falls back; kOriented: so does one whose hinted face the rule rejects)
            if (hg >= 0 && hg < G && d < __builtin_huge_valf() &&
                (!kOriented || !nm.constrained || cp_admissible(t, nm.x, nm.y, nm.z, nm.nn, c2))) {
                hinted = true;
                seed = hg;
                key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)h;
            }
        }
    }
    // sweep 1: an upper bound of the answer, and the group that gives it (this lane's seed); not for a hinted lane, and
    // not at all where every query of the wavefront is hinted
    float ub = __builtin_huge_valf();
    if (!kOriented) {
        if (!kHinted || __ballot(active && !hinted) != 0ull)
            for (int g = 0; g < G; ++g) {
                float lb, far;
                cp_box(px, py, pz, box + (size_t)g * kCpBox, lb, far);
                if (far < ub && !(kHinted && hinted)) { ub = far; seed = g; }
            }
    } else if (__ballot(active && !hinted) != 0ull) {
        // the bound only from groups wholly admissible for the lane; the nearest mixed group is remembered and is the
        // seed where it is nearer (a seed is only a group tested first: it carries no bound)
        float ub_mixed = __builtin_huge_valf();
        int seed_mixed = -1;
        for (int g = 0; g < G; ++g) {
            float lb, far;
            cp_box(px, py, pz, box + (size_t)g * kCpBox, lb, far);
            const int cls = cp_lane_class(nm, cones, g, c);
            if (cls == 1 && far < ub && !hinted) { ub = far; seed = g; }
            if (cls == 0 && far < ub_mixed && !hinted) { ub_mixed = far; seed_mixed = g; }
        }
        if (ub_mixed < ub) seed = seed_mixed;
    }
    // a lane without a query admits nothing (its bound is below every lb - margin, NaN included)
    float bound = active ? __builtin_fmaf(ub, kCpMargin, ub) : -__builtin_huge_valf();
    if (kHinted && hinted) bound = __uint_as_float((unsigned)(key >> 32));
    int buf = 0, first = 0, n = 0;
    CpStage r;
    // The seeds first: the box bound alone is the size of a group, and a lane that met its near groups late in the
    // walk would test every group within that reach before.  After its seed a lane's bound is an exact distance.
    // Every lane that admits a seed group tests it (under its bound of that moment, which only shrinks), so the walk
    // below may leave the seeds out.
    bool pending = active && seed >= 0;
    for (unsigned long long todo = __ballot(pending); todo != 0ull; todo = __ballot(pending)) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int g = __builtin_amdgcn_readlane(seed, src);
        cp_group_range(group_off, g, F, first, n);
        cp_stage_load(r, body_tris, face_list, first, n, lane);
        cp_stage_store(s_tri[buf], s_fid[buf], r, n, lane);
        __syncthreads();
        float lb, far;
        cp_box(px, py, pz, box + (size_t)g * kCpBox, lb, far);
        bool admit = active && lb - kCpMargin * far <= bound;
        if (kOriented) admit = admit && cp_lane_class(nm, cones, g, c) != 2;
        if (admit) {
            key = cp_test_group<kOriented>(px, py, pz, s_tri[buf], s_fid[buf], n, key, nm, c2);
            bound = __builtin_fminf(bound, __uint_as_float((unsigned)(key >> 32)));
        }
        pending = pending && seed != g;
        buf ^= 1;
    }
    // sweep 2: the other groups in index order
    float lbm = 0.0f;
    int g = cp_next_group<kOriented>(box, G, 0, px, py, pz, bound, active, seed, lbm, nm, cones, c);
    if (g < G) {
        cp_group_range(group_off, g, F, first, n);
        cp_stage_load(r, body_tris, face_list, first, n, lane);
    }
    while (g < G) {
        cp_stage_store(s_tri[buf], s_fid[buf], r, n, lane);
        __syncthreads();
        const float lbm_now = lbm;
        const int n_now = n;
        // the next group's loads, before this group's tests
        g = cp_next_group<kOriented>(box, G, g + 1, px, py, pz, bound, active, seed, lbm, nm, cones, c);
        if (g < G) {
            cp_group_range(group_off, g, F, first, n);
            cp_stage_load(r, body_tris, face_list, first, n, lane);
        }
        if (active && lbm_now <= bound) {
            key = cp_test_group<kOriented>(px, py, pz, s_tri[buf], s_fid[buf], n_now, key, nm, c2);
            bound = __builtin_fminf(bound, __uint_as_float((unsigned)(key >> 32)));
        }
        buf ^= 1;
    }
    if (q >= Q) return;
    const size_t o = (size_t)b * Q + q;
    int face = (int)(unsigned)(key & 0xffffffffull);
    float d2 = __uint_as_float((unsigned)(key >> 32)), b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    if (!active || face < 0 || face >= F) {
        face = -1;
        d2 = __builtin_huge_valf();
    } else {
        // the winner's weights: the same sequence on the same corners
        float t[kCpTri], v, w;
        cp_face_corners(faces, verts + (size_t)b * V * 3, V, face, t);
        cp_eval(px, py, pz, t, v, w);
        b1 = v;
        b2 = w;
        b0 = __builtin_fmaxf((1.0f - v) - w, 0.0f);
    }
    out_d2[o] = d2;
    out_face[o] = face;
    out_bary[o * 3] = b0;
    out_bary[o * 3 + 1] = b1;
    out_bary[o * 3 + 2] = b2;
}

// envelope adjoint: the weights held fixed.  grad_points = 2 g (p - c); rows of the winning face's corners get
// -2 g bary[k] (p - c)
template <bool kFixed>
__global__ __launch_bounds__(256) void cp_bwd_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                     const int32_t* __restrict__ face, const float* __restrict__ bary,
                                                     const float* __restrict__ grad_d2, const int32_t* __restrict__ faces,
                                                     int V, int F, int Q, float* __restrict__ grad_points,
                                                     float* __restrict__ grad_verts, long long* __restrict__ grad_fixed)
{
    const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (q >= Q) return;
    const size_t o = (size_t)b * Q + q;
    const int f = face[o];
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (f >= 0 && f < F) {
        const float g2 = 2.0f * grad_d2[o];
        const float w[3] = {bary[o * 3], bary[o * 3 + 1], bary[o * 3 + 2]};
        int vi[3];
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;
        for (int k = 0; k < 3; ++k) {
            vi[k] = cp_clamp_index(faces[(size_t)f * 3 + k], V);
            const float* x = verts + ((size_t)b * V + vi[k]) * 3;
            cx += w[k] * x[0]; cy += w[k] * x[1]; cz += w[k] * x[2];
        }
        gx = g2 * (points[o * 3] - cx);
        gy = g2 * (points[o * 3 + 1] - cy);
        gz = g2 * (points[o * 3 + 2] - cz);
        if (grad_verts || grad_fixed) fit_scatter_corners<kFixed>(grad_verts, grad_fixed, (size_t)b * V, vi, w, gx, gy, gz);
    }
    if (grad_points) {
        grad_points[o * 3] = gx;
        grad_points[o * 3 + 1] = gy;
        grad_points[o * 3 + 2] = gz;
    }
}

}  // namespace

extern "C" size_t tuch_closest_point_workspace_bytes(const tuch_contact_model* m, int B, int Q, int oriented)
{
    if (!m || B <= 0 || Q <= 0) return 0;
    tuch_ws_scope scope(m->opt.canary != 0);
    return cp_layout(m, B, oriented != 0).total;
}

// what the searching entry points ask of max_angle_cos before anything else: with normals, a cosine in [0, 1)
int tuch_cp_check_cos(const char* name, const float* normals, float max_angle_cos)
{
    TUCH_REQUIRE(!normals || (max_angle_cos >= 0.0f && max_angle_cos < 1.0f),
                 "%s: max_angle_cos %g is not in [0, 1) (the cosine of an angle in (0, 90] degrees)", name, (double)max_angle_cos);
    return TUCH_OK;
}

// every entry point that searches (scan_fit.hip's too): `name` is the one the errors speak of; hint == nullptr launches
// the unhinted instantiation, shift == nullptr leaves the points as they are; normals != nullptr launches the oriented
// forms with max_angle_cos (the workspace then holds the cones); without normals max_angle_cos is not read
int tuch_cp_search(const char* name, const tuch_contact_model* m, const float* verts, const float* points, const float* shift,
                   const float* normals, float max_angle_cos, const int32_t* counts, const int32_t* hint, int B, int Q,
                   float* d2, int32_t* face, float* bary, void* workspace, size_t workspace_bytes, void* stream)
{
    const bool oriented = normals != nullptr;
    if (!oriented) max_angle_cos = 0.0f;
    TUCH_REQUIRE(m && verts && points && d2 && face && bary, "%s: null pointer", name);
    TUCH_REQUIRE(B >= 0 && B <= 65535 && Q >= 0, "%s: bad sizes B=%d Q=%d", name, B, Q);
    if (B == 0 || Q == 0) return TUCH_OK;
    TUCH_REQUIRE(m->cp_groups > 0 && m->cp_group_off && m->cp_face_list && m->cp_face_group, "%s: the model has no face groups",
                 name);
    const size_t need = tuch_closest_point_workspace_bytes(m, B, Q, oriented);
    if (!workspace || workspace_bytes < need) {
        tuch_set_error("%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
        return TUCH_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    tuch_ws_scope scope(m->opt.canary != 0);
    const CpLayout l = scope.record(0, [&] { return cp_layout(m, B, oriented); });
    scope.arm(workspace, m->canary_hits, s);
    float* boxes = (float*)((char*)workspace + l.boxes);
    float* tris = (float*)((char*)workspace + l.tris);
    float* cones = oriented ? (float*)((char*)workspace + l.cones) : nullptr;
    const int G = m->cp_groups;
    hipLaunchKernelGGL(oriented ? cp_group_bounds_kernel<true> : cp_group_bounds_kernel<false>, dim3(G, B), dim3(64), 0, s, verts,
                       (const int32_t*)m->faces, (const int32_t*)m->cp_face_list, (const int32_t*)m->cp_group_off, m->V, m->F, G,
                       boxes, tris, cones);
    // c2 = c * c in float32, once, here (the rule's threshold)
    const float c2 = max_angle_cos * max_angle_cos;
    auto* kernel = oriented ? (hint ? cp_search_kernel<true, true> : cp_search_kernel<false, true>)
                            : (hint ? cp_search_kernel<true, false> : cp_search_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(ceil_div(Q, 64), B), dim3(64), 0, s, points, shift, counts, hint,
                       (const int32_t*)m->cp_face_group, (const float*)boxes, (const float*)tris,
                       (const int32_t*)m->cp_group_off, (const int32_t*)m->cp_face_list, (const int32_t*)m->faces, verts, m->V,
                       m->F, G, Q, d2, face, bary, normals, (const float*)cones, max_angle_cos, c2);
    return tuch_check_launch(name);
}

extern "C" int tuch_closest_point(const tuch_contact_model* m, const float* verts, const float* points, const float* normals,
                                  float max_angle_cos, const int32_t* counts, const int32_t* hint, int B, int Q, float* d2,
                                  int32_t* face, float* bary, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = tuch_cp_check_cos("tuch_closest_point", normals, max_angle_cos);
    if (rc != TUCH_OK) return rc;
    return tuch_cp_search("tuch_closest_point", m, verts, points, nullptr, normals, max_angle_cos, counts, hint, B, Q, d2, face,
                          bary, workspace, workspace_bytes, stream);
}

extern "C" int tuch_closest_point_bwd(const tuch_contact_model* m, const float* verts, const float* points, const int32_t* face,
                                      const float* bary, const float* grad_d2, int B, int Q, float* grad_points,
                                      void* grad_verts_fixed_zeroed, float* grad_verts, void* stream)
{
    TUCH_REQUIRE(m && verts && points && face && bary && grad_d2, "tuch_closest_point_bwd: null pointer");
    TUCH_REQUIRE(B >= 0 && B <= 65535 && Q >= 0, "tuch_closest_point_bwd: bad sizes B=%d Q=%d", B, Q);
    if (B == 0 || Q == 0 || !(grad_points || grad_verts_fixed_zeroed || grad_verts)) return TUCH_OK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ceil_div(Q, 256), B);
    if (grad_verts_fixed_zeroed) {
        hipLaunchKernelGGL(cp_bwd_kernel<true>, grid, dim3(256), 0, s, verts, points, face, bary, grad_d2,
                           (const int32_t*)m->faces, m->V, m->F, Q, grad_points, (float*)nullptr,
                           (long long*)grad_verts_fixed_zeroed);
        if (grad_verts)
            tuch_launch_fixed_to_float((const long long*)grad_verts_fixed_zeroed, grad_verts, (size_t)B * m->V * 3, s);
    } else {
        hipLaunchKernelGGL(cp_bwd_kernel<false>, grid, dim3(256), 0, s, verts, points, face, bary, grad_d2,
                           (const int32_t*)m->faces, m->V, m->F, Q, grad_points, grad_verts, (long long*)nullptr);
    }
    return tuch_check_launch("tuch_closest_point_bwd");
}
