// Nearest point of a static point cloud for moving query points (tuch_point_cloud_build / _nearest / _fit_terms / _grid,
// include/tuch_amd.h): a uniform grid per body, built once per cloud, an exact query, and the model -> scan data term of a
// two-sided fit fused into the query's epilogue.
//
// The rule.  The cloud of body b is the set of VALID points of points[b]: index < counts[b], weight != 0 where weights are
// given, all three coordinates finite.  Any other point is never a neighbour and never computed from (it may be NaN).
// The query is q = x + shift[b], one float32 add per component (no shift: the bits of x).  pc_d2 below is THE squared
// distance of a (query, point) pair: d = q - s per component, d2 = (dx dx + dy dy) + dz dz, every product and sum rounded
// to float32 on its own (no fused operation: numpy float32 reproduces the sequence bit for bit).  The winner is the
// smallest packed key (d2 bits << 32 | index), index being the point's position in the caller's [Q] order: the smallest
// d2, among equal bits the smallest index.  Only a finite d2 can win, and with max_distance tau only d2 <= f32(tau) f32(tau)
// (compared in float32).  A query without winner -- empty cloud, non-finite query, nothing within tau, an entry beyond
// query_counts -- gets index -1 and d2 +inf.  Which cells are visited, in which order, where the build filed a point and
// what the hint says never enters a key, so any conservative pruning gives the bits of the full sweep: a query's outputs
// are the same alone or in a batch, for any order of queries or points, any resolution, eager or replayed.
// There is no gradient with respect to the points of the cloud: they are data.
//
// The structure (build: five launches, no host round trip, no allocation, capturable).
//   tuch_launch_zero_words (common.h)  the cell and block tables of every body <- 0 (a kernel, not a memset: a captured
//                      loop then holds kernel nodes only)
//   pc_header_kernel   one workgroup per body: box and number of the valid points -> header [16 words]: origin (the box's
//                      low corner), cell edge = longest extent / resolution (isotropic; at least kPcMinCell, so a box
//                      without extent is one cell), 1 / edge, dims_k = min(resolution, floor(extent_k / edge) + 1)
//   pc_file_kernel<0>  cell of every valid point (pc_t: t = (s - origin) * inv, truncated and clamped into the dims);
//                      integer vector atomics into the cell table and into the table of 4^3-cell blocks
//   pc_scan_kernel     one workgroup per body: exclusive prefix sum of the cell table in place
//   pc_file_kernel<1>  (x, y, z, original index) into cell order through an atomic cursor (the table entry itself, which
//                      ends as the END of its cell: cell c is [table[c - 1], table[c]), cell 0 starts at 0).  The order
//                      inside a cell depends on atomic arrival; by the key rule no output depends on it.
//
// The query.  There is ONE of each piece, and a form of the query is a choice of sink:
//   pc_walk<Sink>       the walk of the grid (what follows, and the margin below, is about it): one query per lane, 64
//                       consecutive queries of one body per wavefront.  A lane walks the blocks in Chebyshev rings
//                       around the block of its own (clamped) cell; a block is opened when it holds points, its bound
//                       admits it and the sink does not pass it by, then each of its cells likewise, then pc_d2 on the
//                       cell's points, which go to the lane's sink.  The walk ends after ring r when the ring bound
//                       (below) exceeds the sink's bound, or when the grid is exhausted.
//   PcBest              the sink of the plain one-key query: the lane's key and the limit
//   PcOriented          the sink of the oriented one-key query: PcBest that asks a candidate the pair rule (below)
//   PcList              the sink of the k-key query: the lane's k smallest keys, its bound the k-th (below)
//   pc_query<kOriented> a lane's whole one-key query: the starting key (limit, -1), the finite check, the hint, the
//                       walk.  kOriented chooses the sink and nothing else.
//   pc_nearest_kernel<kOriented>, pc_fit_kernel<kOriented>   the query for an entry of `queries` and for a vertex with
//                       the term as its epilogue; the <false> instantiations do not read what only the oriented sink
//                       needs; each has one entry point (normals == nullptr is the plain form).
// Keys are made and read by pc_key / pc_won / pc_key_d2 / pc_key_index alone; pc_entries and pc_entry say which
// entries of a body are queries and what the query of an entry is.
//
// Pruning margin.  Everything is measured in cells: t = fl(fl(x - origin) * inv) for a point s (t_s) and for the query
// (t_q), the SAME two operations.  Undoing them, s - q = (t_s (1 + e_s) - t_q (1 + e_q)) / inv with |e| <= 2.1 u
// (u = 2^-24), so along every axis
//     |s - q| inv  >=  |t_s - t_q| - 2.1 u (|t_s| + |t_q|).
// A point filed in cell c has c <= t_s < c + 1 as COMPUTED -- the cell assignment's own rounding is inside t_s, the bound
// needs no box in space that might miss a point an ulp from a wall -- except in the top cell of a clamped axis, where
// t_s <= resolution (1 + 4 u).  With g = max(0, c - t_q, t_q - (c + 1)) as computed (one rounding) and |t_s| <= R + 1:
//     |s - q| inv  >=  g (1 - u) - 6.1 u (|t_q| + R + 1)  >=  l := g (1 - M) - M (max_k |t_q,k| + R + 2),   M = 2^-20 = 16 u
// (the slack term is taken twice what is needed: it covers its own and l's rounding).  1 / inv >= edge (1 - u), the
// computed e = fl(edge max(l, 0)) <= edge l (1 + u), so the true d2 >= sum e_k^2 (1 - 4 u); THE d2 as computed is
// >= true d2 (1 - 6 u) (one rounding in each difference, one in each product, two in the sums: all RELATIVE, however far
// from the origin the coordinates are, because q and s are given floats).  The bound lb = fl(sum fl(e_k^2)) (1 - M)
// <= sum e_k^2 (1 - 12 u) is therefore <= the computed d2 of every point of the cell, and a cell, a block (c .. c + 4) or
// the rest of the grid (ring r done: every unvisited block has an axis with g >= 4 r) is skipped only when lb > the lane's
// bound -- and lb >= kPcNormal, where float32 products have their relative accuracy.  A slab or a row of blocks or cells
// is skipped by the same test on one or two axes' shares alone (a sum of fewer non-negative terms, rounded: not
// larger).  A query outside the grid needs nothing special (t_q is not clamped for the bound); one whose t_q overflows
// has slack +inf, l = 0 and prunes nothing.
//
// The hint.  hint[b,n] in [0, Q) that names a valid point (checked on the caller's arrays before anything else is
// addressed) whose d2 is finite and within tau, and which the sink admits, enters as an ordinary key -- the exact d2 to
// that point, which the full sweep computes too, so it cannot undercut the sweep's minimum; it only shortens the walk.
// Anything else takes the unhinted path.  hint may alias the index output: a lane reads its own entry before it writes
// it.
//
// k nearest points and normals (tuch_point_cloud_knn / _normals; PcList, pc_knn_kernel, pc_normals_kernel).  The
// rule above, verbatim, for the k (1 .. 32) smallest keys of a query in ascending order: index [B,N,k], d2 [B,N,k]; with
// fewer than k admissible points (finite d2, within tau) the tail is -1 / +inf; a non-finite query, an empty cloud or
// an entry beyond query_counts gives all -1 / +inf.  A point that coincides with the query is an ordinary neighbour with
// d2 = 0.  The outputs equal a sorted float32 brute-force sweep bit for bit, alone or in a batch, for any order of
// queries or points, any resolution, eager or replayed.
//   It is pc_walk with the list as its sink: the pruning bound is the lane's k-th key so far; while its list is not full
// the bound is (limit, -1).  The derivation above holds for any such bound: a cell, a block, a row, a slab or the rest
// of the grid is skipped only when its lower bound exceeds the bound's d2, so no point whose key is below the bound is
// ever skipped, and the k smallest keys are found whatever was visited in whatever order.  With no tau the ring test
// cannot end the walk before the list is full (limit is then the largest finite float): the walk ends after a ring
// only once the list is full (or nothing beyond the ring is within tau), or when the grid is exhausted.
//   The list needs dynamic indexing, so it lives in LDS, not in registers: [k][lanes] 64-bit keys (PcList).  It fills in
// arrival order; once full it is a binary max-heap whose root, the bound, is kept in a register.  An accepted candidate
// takes the root's place and sifts down (at most 2 log2 k reads; accepts become rare once the list has warmed up); after
// the walk the lane sorts its keys in place (heap sort) and writes them.  The first form kept the list unsorted with the
// slot of its maximum and rescanned all k slots after every accept; the heap gives the same bits and measured 2.1 x faster
// at k = 32 and 100 000 points (1.4 x at 6 890), 1.1 - 1.4 x at k = 16 and 3 - 10 % slower at k = 8 (DESIGN.md
// section 3).  One launch, no atomics, no cross-lane traffic, no workspace beyond the cloud's: capturable.
//   Neighbourhood statistics, one fixed float32 sequence under this file's contract(off), n <= k neighbours in key order,
// re-read from the caller's `points` by index (clamped): d_j = s_j - q per component; m = (...((d_1 + d_2) + d_3)... +
// d_n) / (float)n; e_j = d_j - m; C_xx, C_xy, C_xz, C_yy, C_yz, C_zz each 0 + e_1,a e_1,b + e_2,a e_2,b + ... left to
// right.  The list is sorted by key, so C has the same bits whatever the grid, the batch or the filing order.  The
// normal is the unit eigenvector of C's smallest eigenvalue (Jacobi, a fixed number of sweeps: above pc_rotate, with
// the derivation of the error bound E and of the zero rows); variation = lambda0 / (lambda0 + lambda1 + lambda2), 0
// where the normal is zero; count = n.  Sign: first canonical (the component of the largest magnitude positive, the
// first among equals); then, with a viewpoint c, t = c - q, s = (n_x t_x + n_y t_y) + n_z t_z, negated when s < 0 (kept
// when s >= 0 or not finite).  Weights decide validity only; the PCA is unweighted.
//
// The term (pc_fit_kernel; tuch_point_cloud_fit_terms): the query for q = verts[b,v] + transl[b], then per vertex
// g_v = scale w_v rho'(d2_v) / sum w and grad_verts[b,v] = 2 g_v (q - s) written by the lane that owns the row (no
// atomics); the per-body loss, the normaliser and grad_transl = sum_v grad_verts[b,v] cross to the workgroup that
// arrives last through fit_reduce_tail (fit_reduce.h: the hand-over all three fit terms use, drained write-through
// stores and no fences, and its argument) and are added in chunk order, the total in a fixed tree: no float atomics,
// the same bits in either mode of tuch_set_deterministic and for a body alone or in a batch.  The normaliser is
// fit_body_sum, rho is fit_rho.  A vertex of weight 0 is not computed from; one without winner contributes rho(tau^2)
// when tau is given and the cloud is not empty, else 0, with a zero gradient row; a body with an empty cloud or without
// weight has loss 0.
//
// The oriented query (tuch_point_cloud_nearest / _fit_terms with normals, _build_cones) is the query above with
// another sink, PcOriented: the same key, pc_d2, walk, margin, hint and outputs, over the ADMISSIBLE valid points only.
// Points carry normals n (caller's order, never filed), a query a normal u: an entry of query_normals, or, in the
// term, what the lane that owns vertex v forms itself from the UNTRANSLATED verts by vn_vertex_normal (face_normal.h;
// tuch_vertex_normals' raw row).  pc_admissible is THE admissibility of a pair, stated in include/tuch_amd.h: with
// uu = |u|^2, nn = |n|^2, s = u . n, every operation rounded to float32 on its own,
//     admissible <=> s > 0 and s s >= c2 (uu nn),  c2 = c c;
// a pair whose uu or nn is 0 or not finite is unconstrained, so a call whose query normals or point normals are all
// zero has the plain call's bits.  The rule is a function of the pair's bits and c alone, so the admissible set of a
// query never depends on cell, lane, batch or order, and the winner -- the smallest key over the admissible valid
// points -- is the full sweep's whatever is pruned conservatively.  The sink asks a candidate the rule only when it
// would otherwise become the best (d2 <= limit and key < best), so its bound is always the key of an admissible point
// (or the limit) and every argument of the pruning margin above holds unchanged.  Likewise the hint: it seeds the
// bound only if the sink admits it, and then its key is one the sweep computes too.
//   What it costs.  A lane whose admissible match is far away, or that has none, finds the key above every nearer
// inadmissible point and gathers that point's normal (12 bytes at a random place) to refuse it; such lanes are a sixth
// to a half of a body's vertices on a scan that sees one side.  The cones below take whole blocks off that path;
// DESIGN.md section 3 has the measured times, which say that they are not enough.
//   The cones.  pc_cones_kernel stores per (body, 4^3-cell block) closest_point.hip's cone record (face_normal.h) over
// the normals of the points filed in the block: an axis A (the normalised mean of the unit normals n / |n|), cos beta
// and sin beta of the normal that makes the largest angle beta with A, the smallest and largest nn, and a flag: usable
// only if the block holds a point, every point's nn is in [kCpSaneLo, kCpSaneHi] -- so a block that holds ANY
// unconstrained point (a zero or non-finite row) is never usable, never skipped -- and the mean has a direction.
// Nothing in it depends on the queries.  With alpha the angle between A and u, every normal of the block makes an angle
// of at least alpha - beta with u; cp_cone_class (the one function the face groups use) says "wholly inadmissible"
//     if  cos alpha < cos beta - kCpConeMargin  (alpha > beta)  and  cos(alpha - beta) <= c - kCpConeMargin
// (0 < alpha - beta <= 180 deg, where the cosine is monotone: alpha - beta > max_angle, no normal of the block is within
// max_angle of u), and only for a lane with kCpNormalLo <= uu <= kCpNormalHi and kCpPairLo <= uu nn <= kCpPairHi for the
// block's extreme nn; any other lane skips nothing.  The margin is closest_point.hip's, its derivation carries over
// term by term with (m, n) read as (n, u): the rule is the same sequence of operations on a pair of vectors (there m is
// computed, here n is given, which only removes an error source), so it decides "cos angle(n, u) >= c" with the
// threshold moved by less than 8 u; A, n / |n| and u / |u| are unit vectors to 3 u each, cos alpha, sin alpha, cos beta,
// sin beta (cross products, not sqrt(1 - cos^2)) within 10 u, cos(alpha - beta) within 43 u: 51 u against the margin's
// 256 u.  (The axis is a MEAN, so its squared length is at most 1 however many points a block holds; which axis is
// taken affects how often a block is skipped, never whether skipping is right: beta is measured against the axis
// actually stored.)  A skipped block holds no admissible point for the lane, so no key of the admissible set is lost:
// the cones only skip, they never decide, and the bits are those of the call with cones NULL.  The buffer starts with
// a header (the resolution the cones were built at): a lane uses them only if that is the cloud's resolution and its
// body's records lie inside the buffer.  They are stale after the next build.
#include "face_normal.h"
#include "fit_reduce.h"
#include "workspace.h"
#include <math.h>
#include <string.h>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = kFitBlock;
constexpr int kCtl = 64;                 // control words in front of the headers: [0] guard words found changed
constexpr int kHead = 16;                // words per body header
constexpr int kMaxRes = 256;
constexpr float kPcMargin = 9.5367431640625e-7f;       // M = 2^-20
constexpr float kPcMinCell = 1e-6f;
constexpr float kPcNormal = 1e-30f;
constexpr float kPcMaxD2 = 3.402823466e+38f;             // the largest finite d2: only a finite d2 can win
constexpr unsigned long long kPcNoKey = 0x7f800000ffffffffull;      // d2 = +inf, index = -1

enum { H_OX = 0, H_OY, H_OZ, H_CELL, H_INV, H_DX, H_DY, H_DZ, H_N, H_RES };

int g_pc_canary = 0;

struct PcLayout { size_t head, sorted, tables, total; };

// ints per body in the tables: the cells, then the 4^3-cell blocks
__host__ __device__ inline size_t pc_table_ints(int R)
{
    const size_t c = (size_t)((R + 3) >> 2);
    return (size_t)R * R * R + c * c * c;
}

// resolution 0: the regions a query addresses by themselves (the tables come last, their extent is on the device)
PcLayout pc_layout(int B, int Q, int R)
{
    PcLayout l;
    size_t o = 0;
    l.head = tuch_ws_take(o, ((size_t)kCtl + (size_t)B * kHead) * sizeof(uint32_t));
    l.sorted = tuch_ws_take(o, (size_t)B * Q * 4 * sizeof(float));
    l.tables = tuch_ws_take(o, (size_t)B * pc_table_ints(R) * sizeof(int32_t));
    l.total = o;
    return l;
}

struct PcScratch { size_t partial, total; };

PcScratch pc_scratch(int B, int N)
{
    PcScratch l;
    size_t o = 0;
    l.partial = tuch_ws_take(o, (size_t)B * ceil_div(N, kBlock) * kFitPart * sizeof(float));
    l.total = o;
    return l;
}

static __device__ __forceinline__ int pc_clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }
static __device__ __forceinline__ bool pc_finite3(float x, float y, float z)
{
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// One float32 operation, rounded on its own.  Plain operators under this file's contract(off): the __f*_rn functions of
// the HIP headers are compiled under the headers' own contraction mode and fuse after inlining.
static __device__ __forceinline__ float pc_mul(float a, float b) { return a * b; }
static __device__ __forceinline__ float pc_add(float a, float b) { return a + b; }
static __device__ __forceinline__ float pc_sub(float a, float b) { return a - b; }

// THE squared distance
static __device__ __forceinline__ float pc_d2(float qx, float qy, float qz, float sx, float sy, float sz)
{
    const float dx = pc_sub(qx, sx), dy = pc_sub(qy, sy), dz = pc_sub(qz, sz);
    return pc_add(pc_add(pc_mul(dx, dx), pc_mul(dy, dy)), pc_mul(dz, dz));
}

// THE key of a (d2, index) pair: the smaller key is the nearer point, among equal d2 bits the smaller index.  A key whose
// index is -1 names no point (the starting key, kPcNoKey): the query has not won.
static __device__ __forceinline__ unsigned long long pc_key(float d2, int index)
{
    return ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)index;
}
static __device__ __forceinline__ float pc_key_d2(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
static __device__ __forceinline__ int pc_key_index(unsigned long long key) { return (int32_t)(uint32_t)key; }
static __device__ __forceinline__ bool pc_won(unsigned long long key) { return (uint32_t)key != 0xffffffffu; }
// is point i of body b in the cloud?  (its coordinates only where it may be)
static __device__ __forceinline__ bool pc_valid(const float* __restrict__ points, const int32_t* __restrict__ counts,
                                                const float* __restrict__ weights, int b, int Q, int i, float& x, float& y,
                                                float& z)
{
    int count = Q;
    if (counts) count = pc_clampi(counts[b], 0, Q);
    if (i < 0 || i >= count) return false;
    const size_t o = (size_t)b * Q + i;
    if (weights && weights[o] == 0.0f) return false;
    x = points[o * 3]; y = points[o * 3 + 1]; z = points[o * 3 + 2];
    return pc_finite3(x, y, z);
}

// Entry i of body b of queries [B][N][3] as a query.  pc_entries: how many entries of the body are queries (the rest
// have no winner and are not read); pc_entry: q = x + shift[b], one add per component (no shift: the bits of x).
static __device__ __forceinline__ int pc_entries(const int32_t* __restrict__ query_counts, int b, int N)
{
    return query_counts ? pc_clampi(query_counts[b], 0, N) : N;
}
template <bool kShifted = false>
static __device__ __forceinline__ void pc_entry(const float* __restrict__ queries, const float* __restrict__ shift, int b, int N,
                                                int i, float& qx, float& qy, float& qz)
{
    const size_t o = (size_t)b * N + i;
    qx = queries[o * 3]; qy = queries[o * 3 + 1]; qz = queries[o * 3 + 2];
    if (kShifted || shift) {
        qx = pc_add(qx, shift[3 * b]); qy = pc_add(qy, shift[3 * b + 1]); qz = pc_add(qz, shift[3 * b + 2]);
    }
}

struct PcGrid {
    float ox, oy, oz, cell, inv;
    int dx, dy, dz, cdx, cdy, cdz, n, res;
};

static __device__ __forceinline__ PcGrid pc_grid(const uint32_t* __restrict__ head, int b)
{
    const uint32_t* h = head + kCtl + (size_t)b * kHead;
    PcGrid g;
    g.ox = __uint_as_float(h[H_OX]); g.oy = __uint_as_float(h[H_OY]); g.oz = __uint_as_float(h[H_OZ]);
    g.cell = __uint_as_float(h[H_CELL]); g.inv = __uint_as_float(h[H_INV]);
    g.res = pc_clampi((int)h[H_RES], 1, kMaxRes);
    g.dx = pc_clampi((int)h[H_DX], 1, g.res); g.dy = pc_clampi((int)h[H_DY], 1, g.res); g.dz = pc_clampi((int)h[H_DZ], 1, g.res);
    g.cdx = (g.dx + 3) >> 2; g.cdy = (g.dy + 3) >> 2; g.cdz = (g.dz + 3) >> 2;
    g.n = (int)h[H_N];
    return g;
}

// a coordinate in cells, as the build and the query both compute it
static __device__ __forceinline__ float pc_t(float x, float o, float inv) { return pc_mul(pc_sub(x, o), inv); }
// the cell of a coordinate in cells, clamped into the axis (t >= 0 for a point of the box; NaN cannot occur for one)
static __device__ __forceinline__ int pc_axis_cell(float t, int d)
{
    return pc_clampi((int)__builtin_fminf(__builtin_fmaxf(t, 0.0f), (float)(d - 1)), 0, d - 1);
}

__global__ __launch_bounds__(kBlock) void pc_header_kernel(const float* __restrict__ points, const int32_t* __restrict__ counts,
                                                          const float* __restrict__ weights, int Q, int R,
                                                          uint32_t* __restrict__ head)
{
    __shared__ float lo[3][kBlock], hi[3][kBlock];
    __shared__ int cnt[kBlock];
    const int b = blockIdx.x, t = threadIdx.x;
    const float inf = __builtin_inff();
    float l[3] = {inf, inf, inf}, h[3] = {-inf, -inf, -inf};
    int n = 0;
    for (int i = t; i < Q; i += kBlock) {
        float x, y, z;
        if (pc_valid(points, counts, weights, b, Q, i, x, y, z)) {
            l[0] = __builtin_fminf(l[0], x); l[1] = __builtin_fminf(l[1], y); l[2] = __builtin_fminf(l[2], z);
            h[0] = __builtin_fmaxf(h[0], x); h[1] = __builtin_fmaxf(h[1], y); h[2] = __builtin_fmaxf(h[2], z);
            ++n;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k][t] = l[k]; hi[k][t] = h[k]; }
    cnt[t] = n;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo[k][t] = __builtin_fminf(lo[k][t], lo[k][t + s]);
                hi[k][t] = __builtin_fmaxf(hi[k][t], hi[k][t + s]);
            }
            cnt[t] += cnt[t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    uint32_t* out = head + kCtl + (size_t)b * kHead;
    float o[3] = {0.0f, 0.0f, 0.0f}, cell = 1.0f;
    int d[3] = {1, 1, 1};
    const int total = cnt[0];
    if (total > 0) {
        float e[3], em = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = lo[k][0];
            e[k] = pc_sub(hi[k][0], lo[k][0]);
            em = __builtin_fmaxf(em, e[k]);
        }
        cell = em / (float)R;
        if (!(cell >= kPcMinCell)) cell = kPcMinCell;
        if (!(cell <= 1e30f)) cell = 1e30f;
        const float inv = 1.0f / cell;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d[k] = pc_clampi((int)__builtin_fminf(pc_mul(e[k], inv), (float)R) + 1, 1, R);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { out[H_OX + k] = __float_as_uint(o[k]); out[H_DX + k] = (uint32_t)d[k]; }
    out[H_CELL] = __float_as_uint(cell);
    out[H_INV] = __float_as_uint(1.0f / cell);
    out[H_N] = (uint32_t)total;
    out[H_RES] = (uint32_t)R;
    for (int k = H_RES + 1; k < kHead; ++k) out[k] = 0u;
}

template <bool kScatter>
__global__ __launch_bounds__(kBlock) void pc_file_kernel(const float* __restrict__ points, const int32_t* __restrict__ counts,
                                                        const float* __restrict__ weights, int Q, int R,
                                                        const uint32_t* __restrict__ head, int32_t* __restrict__ tables,
                                                        float4* __restrict__ sorted)
{
    const int b = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
    float x, y, z;
    if (i >= Q || !pc_valid(points, counts, weights, b, Q, i, x, y, z)) return;
    const PcGrid g = pc_grid(head, b);
    const int cx = pc_axis_cell(pc_t(x, g.ox, g.inv), g.dx), cy = pc_axis_cell(pc_t(y, g.oy, g.inv), g.dy),
              cz = pc_axis_cell(pc_t(z, g.oz, g.inv), g.dz);
    const size_t fine = (size_t)R * R * R;
    int32_t* tab = tables + (size_t)b * pc_table_ints(R);
    const int c = (cz * g.dy + cy) * g.dx + cx;                 // < R^3
    if (kScatter) {
        const int pos = pc_clampi(atomicAdd(tab + c, 1), 0, Q - 1);
        sorted[(size_t)b * Q + pos] = make_float4(x, y, z, __int_as_float(i));
    } else {
        atomicAdd(tab + c, 1);
        atomicAdd(tab + fine + ((cz >> 2) * g.cdy + (cy >> 2)) * g.cdx + (cx >> 2), 1);
    }
}

// exclusive prefix sum of a body's cell counts, in place: thread t owns the cells [t per, (t + 1) per)
__global__ __launch_bounds__(kBlock) void pc_scan_kernel(const uint32_t* __restrict__ head, int R, int32_t* __restrict__ tables)
{
    __shared__ int sums[kBlock];
    const int b = blockIdx.x, t = threadIdx.x;
    const PcGrid g = pc_grid(head, b);
    int32_t* tab = tables + (size_t)b * pc_table_ints(R);
    const int cells = g.dx * g.dy * g.dz;                       // <= R^3 (the dims are clamped to R)
    const int per = (cells + kBlock - 1) / kBlock;
    const int from = t * per < cells ? t * per : cells, to = from + per < cells ? from + per : cells;
    int acc = 0;
    for (int c = from; c < to; ++c) acc += tab[c];
    sums[t] = acc;
    __syncthreads();
    for (int s = 1; s < kBlock; s <<= 1) {                      // inclusive scan of the threads' sums
        const int v = t >= s ? sums[t - s] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int run = sums[t] - acc;
    for (int c = from; c < to; ++c) {
        const int v = tab[c];
        tab[c] = run;
        run += v;
    }
}

// ---------------------------------------------------------------------------------------------------------- the query
struct PcTables {
    const uint32_t* head;
    const float4* sorted;        // [B][Q]
    const int32_t* tables;       // [B][res^3 + blocks]
    long long cap;               // ints behind `tables` that belong to the workspace
};

static __device__ __forceinline__ int pc_table(const PcTables& w, long long at)
{
    return w.tables[at < 0 ? 0 : (at >= w.cap ? w.cap - 1 : at)];
}

// lower bound of the squared distance to anything filed in the cells [c0, c1) of one axis, in cells: max(l, 0)
static __device__ __forceinline__ float pc_gap(float tq, int c0, int c1, float slack)
{
    const float g = __builtin_fmaxf(__builtin_fmaxf(pc_sub((float)c0, tq), pc_sub(tq, (float)c1)), 0.0f);
    return __builtin_fmaxf(pc_sub(pc_mul(g, 1.0f - kPcMargin), slack), 0.0f);
}
static __device__ __forceinline__ float pc_sq(float cell, float l)
{
    const float e = pc_mul(cell, l);
    return pc_mul(e, e);
}
// is everything behind this bound out of reach of the key?
static __device__ __forceinline__ bool pc_out(float sum, unsigned long long best)
{
    const float lb = pc_mul(sum, 1.0f - kPcMargin);
    return lb > pc_key_d2(best) && lb >= kPcNormal;
}

// The sink of a one-key query: `best` arrives as the starting key (no key: (limit bits, -1) with limit = tau^2 or
// FLT_MAX; or the hinted key) and ends as the smallest key.  A candidate needs d2 <= limit.
struct PcBest {
    unsigned long long best;
    float limit;
    __device__ __forceinline__ unsigned long long bound() const { return best; }
    __device__ __forceinline__ void offer(float d2, unsigned long long key)
    {
        best = d2 <= limit && key < best ? key : best;         // (a select, not a branch around a store: the innermost loop)
    }
    __device__ __forceinline__ bool skip_block(long long) const { return false; }
    __device__ __forceinline__ bool admits(int) const { return true; }
};

// what the oriented query knows of the cloud's normals
struct PcOrient {
    const float* normals;        // [B][Q][3], the caller's order
    const uint32_t* cones;       // kCpCone header words ([0]: the resolution they were built at), then the records; or nullptr
    long long cone_cap;          // records behind the header
    float c, c2;                 // the cosine and its square
};

// THE admissibility of a (query normal u, point normal n) pair (file header: the oriented query): every operation
// rounded on its own.  uu is the caller's (ux ux + uy uy) + uz uz, positive and finite; a point whose nn is 0 or not
// finite has no normal and is admissible.
static __device__ __forceinline__ bool pc_admissible(float ux, float uy, float uz, float uu, float nx, float ny, float nz,
                                                     float c2)
{
    const float nn = pc_add(pc_add(pc_mul(nx, nx), pc_mul(ny, ny)), pc_mul(nz, nz));
    if (!(nn > 0.0f && __builtin_isfinite(nn))) return true;
    const float s = pc_add(pc_add(pc_mul(ux, nx), pc_mul(uy, ny)), pc_mul(uz, nz));
    return s > 0.0f && pc_mul(s, s) >= pc_mul(c2, pc_mul(uu, nn));
}

// The sink of the oriented one-key query: PcBest with the pair rule asked of a candidate that would otherwise become
// the best -- rare once the key has settled, so the gather from the caller-order normals stays out of the innermost
// loop's common path -- and with the block cones (file header).  normals: the body's [Q][3]; cones: the body's records
// or nullptr (none, or this lane may not use them).
struct PcOriented {
    unsigned long long best;
    float limit;
    const float* normals;
    int Q;
    float ux, uy, uz, uu, c2;
    bool constrained;            // uu is positive and finite: the rule applies (otherwise every point is admissible)
    const float* cones;
    long long cone_cap;
    float inv, c;                // 1 / |u| and the cosine, for the cones
    // Everything but the key and the limit, for the query normal u of a lane of body b.  The cones serve the lane only
    // if they were built at the cloud's resolution, lie wholly inside the buffer for its body, and uu is in the sane
    // range (file header).
    __device__ __forceinline__ void orient(const PcTables& w, const PcOrient& o, int b, int Q_, float ux_, float uy_, float uz_)
    {
        normals = o.normals + (size_t)b * Q_ * 3;
        Q = Q_;
        ux = ux_; uy = uy_; uz = uz_;
        uu = pc_add(pc_add(pc_mul(ux, ux), pc_mul(uy, uy)), pc_mul(uz, uz));
        c2 = o.c2; c = o.c;
        constrained = uu > 0.0f && __builtin_isfinite(uu);
        cones = nullptr; cone_cap = 1; inv = 0.0f;
        if (o.cones && constrained && uu >= kCpNormalLo && uu <= kCpNormalHi) {
            const int res = pc_clampi((int)w.head[kCtl + (size_t)b * kHead + H_RES], 1, kMaxRes), cres = (res + 3) >> 2;
            const long long stride = (long long)cres * cres * cres;
            if ((int)o.cones[0] == res && (b + 1) * stride <= o.cone_cap) {
                cones = (const float*)(o.cones + kCpCone) + (size_t)b * stride * kCpCone;
                cone_cap = stride;
                inv = 1.0f / __builtin_sqrtf(uu);
            }
        }
    }
    __device__ __forceinline__ unsigned long long bound() const { return best; }
    __device__ __forceinline__ bool admits(int index) const
    {
        if (!constrained) return true;
        const float* n = normals + (size_t)pc_clampi(index, 0, Q - 1) * 3;
        return pc_admissible(ux, uy, uz, uu, n[0], n[1], n[2], c2);
    }
    __device__ __forceinline__ void offer(float d2, unsigned long long key)
    {
        if (d2 <= limit && key < best && admits(pc_key_index(key))) best = key;
    }
    // may the lane pass block `block` of its body by?  Only a usable cone that is wholly inadmissible for u says so.
    __device__ __forceinline__ bool skip_block(long long block) const
    {
        if (!cones) return false;
        const long long at = block < 0 ? 0 : (block >= cone_cap ? cone_cap - 1 : block);
        return cp_cone_class(cones + (size_t)at * kCpCone, ux, uy, uz, inv, c) == 2;
    }
};

// THE walk of the grid, for the finite query (qx, qy, qz) against the cloud of body b: the rings, gaps, slack and 2^-20
// margin of the file header.  Everything is pruned against sink.bound(), a key that no candidate still wanted lies
// above (PcBest: the best key so far; PcList below: the k-th), and every point of a cell that is opened goes to
// sink.offer(d2, key).  The sink comes and goes by value: it lives in registers, and pc_nearest_kernel<false> compiles
// to the instructions it had when the walk was written out for the one key.
template <typename Sink>
static __device__ Sink pc_walk(const PcTables& w, int b, int Q, float qx, float qy, float qz, Sink sink)
{
    const PcGrid g = pc_grid(w.head, b);
    const int n = pc_clampi(g.n, 0, Q);
    if (n == 0) return sink;
    const long long fine = (long long)g.res * g.res * g.res;
    const int cres = (g.res + 3) >> 2;
    const long long base = (long long)b * (fine + (long long)cres * cres * cres);
    const float4* pts = w.sorted + (size_t)b * Q;
    const float tx = pc_t(qx, g.ox, g.inv), ty = pc_t(qy, g.oy, g.inv), tz = pc_t(qz, g.oz, g.inv);
    const float tmax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(tx), __builtin_fabsf(ty)), __builtin_fabsf(tz));
    const float slack = pc_mul(kPcMargin, pc_add(tmax, (float)(g.res + 2)));
    const int hx = pc_axis_cell(tx, g.dx) >> 2, hy = pc_axis_cell(ty, g.dy) >> 2, hz = pc_axis_cell(tz, g.dz) >> 2;
    int rmax = hx > g.cdx - 1 - hx ? hx : g.cdx - 1 - hx;
    rmax = rmax > hy ? rmax : hy;
    rmax = rmax > g.cdy - 1 - hy ? rmax : g.cdy - 1 - hy;
    rmax = rmax > hz ? rmax : hz;
    rmax = rmax > g.cdz - 1 - hz ? rmax : g.cdz - 1 - hz;
    for (int r = 0; r <= rmax; ++r) {
        // rings 0 .. r - 1 are done: every block left has an axis with g >= 4 (r - 1)
        if (r > 1 && pc_out(pc_sq(g.cell, pc_gap(0.0f, 4 * (r - 1), 4 * (r - 1) + 1, slack)), sink.bound())) break;
        const int z0 = hz - r < 0 ? 0 : hz - r, z1 = hz + r > g.cdz - 1 ? g.cdz - 1 : hz + r;
        const int y0 = hy - r < 0 ? 0 : hy - r, y1 = hy + r > g.cdy - 1 ? g.cdy - 1 : hy + r;
        const int x0 = hx - r < 0 ? 0 : hx - r, x1 = hx + r > g.cdx - 1 ? g.cdx - 1 : hx + r;
        for (int bz = z0; bz <= z1; ++bz) {
            const float lz = pc_sq(g.cell, pc_gap(tz, 4 * bz, 4 * bz + 4, slack));
            if (pc_out(lz, sink.bound())) continue;                          // (one axis' share alone: the whole slab is out)
            const bool zface = bz - hz == r || hz - bz == r;
            for (int by = y0; by <= y1; ++by) {
                const float lyz = pc_add(pc_sq(g.cell, pc_gap(ty, 4 * by, 4 * by + 4, slack)), lz);
                if (pc_out(lyz, sink.bound())) continue;
                const bool face = zface || by - hy == r || hy - by == r;
                // the shell of the ring: whole rows on its faces, else the two end blocks
                const int step = face ? 1 : 2 * r;
                for (int bx = face ? x0 : (hx - r >= 0 ? hx - r : hx + r); bx <= x1; bx += step) {
                    if (pc_table(w, base + fine + ((long long)bz * g.cdy + by) * g.cdx + bx) <= 0) continue;
                    // (the sum's order differs from a cell's below; both are bounds of their own)
                    if (pc_out(pc_add(pc_sq(g.cell, pc_gap(tx, 4 * bx, 4 * bx + 4, slack)), lyz), sink.bound())) continue;
                    if (sink.skip_block(((long long)bz * g.cdy + by) * g.cdx + bx)) continue;    // (the oriented sink's cones)
                    const int cz1 = 4 * bz + 4 < g.dz ? 4 * bz + 4 : g.dz, cy1 = 4 * by + 4 < g.dy ? 4 * by + 4 : g.dy,
                              cx1 = 4 * bx + 4 < g.dx ? 4 * bx + 4 : g.dx;
                    for (int cz = 4 * bz; cz < cz1; ++cz) {
                        const float mz = pc_sq(g.cell, pc_gap(tz, cz, cz + 1, slack));
                        if (pc_out(mz, sink.bound())) continue;
                        for (int cy = 4 * by; cy < cy1; ++cy) {
                            const float myz = pc_add(pc_sq(g.cell, pc_gap(ty, cy, cy + 1, slack)), mz);
                            if (pc_out(myz, sink.bound())) continue;
                            const long long row = base + ((long long)cz * g.dy + cy) * g.dx;
                            for (int cx = 4 * bx; cx < cx1; ++cx) {
                                const long long c = row + cx;
                                const int end = pc_clampi(pc_table(w, c), 0, n);
                                const int begin = c == base ? 0 : pc_clampi(pc_table(w, c - 1), 0, n);
                                if (begin >= end) continue;
                                if (pc_out(pc_add(pc_sq(g.cell, pc_gap(tx, cx, cx + 1, slack)), myz), sink.bound())) continue;
                                for (int p = begin; p < end; ++p) {
                                    const float4 s = pts[p];
                                    const float d2 = pc_d2(qx, qy, qz, s.x, s.y, s.z);
                                    sink.offer(d2, pc_key(d2, __float_as_int(s.w)));
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    return sink;
}

// The whole query of one lane, plain or oriented: the starting key, the hint, the search.  Returns the key; !pc_won(key):
// no winner.  kOriented only chooses the sink (PcOriented, set up for the query normal u) and with it what the hint is
// asked besides validity and the limit: PcBest admits every point.  The plain form reads neither `o` nor u.
template <bool kOriented>
static __device__ __forceinline__ unsigned long long pc_query(const PcTables& w, const PcOrient& o,
                                                              const float* __restrict__ points,
                                                              const int32_t* __restrict__ counts,
                                                              const float* __restrict__ weights, int b, int Q, float qx,
                                                              float qy, float qz, float ux, float uy, float uz, int hint,
                                                              float limit)
{
    std::conditional_t<kOriented, PcOriented, PcBest> sink;
    sink.best = pc_key(limit, -1);
    sink.limit = limit;
    if (!pc_finite3(qx, qy, qz)) return sink.best;
    if constexpr (kOriented) sink.orient(w, o, b, Q, ux, uy, uz);
    float sx, sy, sz;
    if (hint >= 0 && hint < Q && pc_valid(points, counts, weights, b, Q, hint, sx, sy, sz)) {
        const float d2 = pc_d2(qx, qy, qz, sx, sy, sz);
        if (d2 <= limit && sink.admits(hint)) sink.best = pc_key(d2, hint);
    }
    return pc_walk(w, b, Q, qx, qy, qz, sink).best;
}

// tuch_point_cloud_nearest; kOriented: with normals (kOriented = false: orient and query_normals are not read)
template <bool kOriented>
__global__ __launch_bounds__(kBlock) void pc_nearest_kernel(PcTables w, PcOrient orient, const float* __restrict__ points,
                                                           const int32_t* __restrict__ counts,
                                                           const float* __restrict__ weights,
                                                           const float* __restrict__ queries,
                                                           const float* __restrict__ query_normals,
                                                           const float* __restrict__ shift,
                                                           const int32_t* __restrict__ query_counts, const int32_t* hint,
                                                           float limit, int Q, int N, float* __restrict__ d2_out,
                                                           int32_t* index_out)
{
    const int b = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const size_t o = (size_t)b * N + i;
    unsigned long long best = kPcNoKey;
    if (i < pc_entries(query_counts, b, N)) {
        const int h = hint ? hint[o] : -1;
        float qx, qy, qz, ux = 0.0f, uy = 0.0f, uz = 0.0f;
        pc_entry(queries, shift, b, N, i, qx, qy, qz);
        if constexpr (kOriented) { ux = query_normals[o * 3]; uy = query_normals[o * 3 + 1]; uz = query_normals[o * 3 + 2]; }
        best = pc_query<kOriented>(w, orient, points, counts, weights, b, Q, qx, qy, qz, ux, uy, uz, h, limit);
    }
    const bool won = pc_won(best);
    d2_out[o] = won ? pc_key_d2(best) : __builtin_inff();
    index_out[o] = won ? pc_key_index(best) : -1;
}

// ----------------------------------------------------------------------------------------------------------- the cones
// The cone of one 4^3-cell block of one body (file header: the cones): one wavefront per block, its lanes striding over
// the block's points row by row (the four cells of a block's row are contiguous in the filed order).  The record is
// closest_point.hip's: axis (the normalised mean of the unit normals), cos beta and sin beta of the normal farthest from
// it, usable, the smallest and the largest nn.  Not usable -- never skipped -- when the block is empty, holds a point
// whose nn is outside [kCpSaneLo, kCpSaneHi] (zero rows, the "unknown" normals, and non-finite ones among them), or
// the mean has no direction.  Lane 0 of block 0 of body 0 writes the header.
__global__ __launch_bounds__(64) void pc_cones_kernel(PcTables w, const float* __restrict__ normals, int Q, int R,
                                                     uint32_t* __restrict__ cones)
{
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x;
    const int cres = (R + 3) >> 2;
    const long long stride = (long long)cres * cres * cres;
    if (b == 0 && blk == 0 && lane < kCpCone) cones[lane] = lane == 0 ? (uint32_t)R : 0u;
    float* rec = (float*)(cones + kCpCone) + ((size_t)b * stride + blk) * kCpCone;
    const PcGrid g = pc_grid(w.head, b);
    const int n = pc_clampi(g.n, 0, Q);
    const long long fine = (long long)g.res * g.res * g.res;
    const long long base = (long long)b * (fine + stride);
    const bool live = g.res == R && blk < g.cdx * g.cdy * g.cdz;
    const int count = live ? pc_clampi(pc_table(w, base + fine + blk), 0, n) : 0;
    if (count <= 0) {
        if (lane < kCpCone) rec[lane] = 0.0f;
        return;
    }
    const int bx = blk % g.cdx, by = (blk / g.cdx) % g.cdy, bz = blk / (g.cdx * g.cdy);
    const float4* pts = w.sorted + (size_t)b * Q;
    const float* body = normals + (size_t)b * Q * 3;
    const float inf = __builtin_inff();
    float ax = 0.0f, ay = 0.0f, az = 0.0f, cb = 2.0f, sb = 0.0f, lo = inf, hi = 0.0f;
    bool sane = true;
    for (int pass = 0; pass < 2; ++pass) {
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (int row = 0; row < 16; ++row) {
            const int cz = 4 * bz + (row >> 2), cy = 4 * by + (row & 3);
            if (cz >= g.dz || cy >= g.dy) continue;
            const long long first = base + ((long long)cz * g.dy + cy) * g.dx + 4 * bx;
            const int cx1 = 4 * bx + 4 < g.dx ? 4 * bx + 4 : g.dx;
            const int begin = first == base ? 0 : pc_clampi(pc_table(w, first - 1), 0, n);
            const int end = pc_clampi(pc_table(w, first + (cx1 - 4 * bx) - 1), 0, n);
            for (int p = begin + lane; p < end; p += 64) {
                const float* nm = body + (size_t)pc_clampi(__float_as_int(pts[p].w), 0, Q - 1) * 3;
                const float nx = nm[0], ny = nm[1], nz = nm[2];
                const float nn = (nx * nx + ny * ny) + nz * nz;
                const bool ok = nn >= kCpSaneLo && nn <= kCpSaneHi;
                const float inv = ok ? 1.0f / __builtin_sqrtf(nn) : 0.0f;
                const float hx = nx * inv, hy = ny * inv, hz = nz * inv;
                if (pass == 0) {
                    sane = sane && ok;
                    sx += hx; sy += hy; sz += hz;
                    lo = __builtin_fminf(lo, ok ? nn : 0.0f); hi = __builtin_fmaxf(hi, ok ? nn : inf);
                } else {
                    const float wx = ay * hz - az * hy, wy = az * hx - ax * hz, wz = ax * hy - ay * hx;
                    const float ca = (ax * hx + ay * hy) + az * hz;
                    if (ca < cb) { cb = ca; sb = __builtin_sqrtf((wx * wx + wy * wy) + wz * wz); }
                }
            }
        }
        if (pass == 0) {
            for (int d = 32; d > 0; d >>= 1) {
                sx += __shfl_xor(sx, d, 64); sy += __shfl_xor(sy, d, 64); sz += __shfl_xor(sz, d, 64);
                lo = __builtin_fminf(lo, __shfl_xor(lo, d, 64)); hi = __builtin_fmaxf(hi, __shfl_xor(hi, d, 64));
            }
            sx = __shfl(sx, 0, 64) / (float)count; sy = __shfl(sy, 0, 64) / (float)count; sz = __shfl(sz, 0, 64) / (float)count;
            const float len2 = (sx * sx + sy * sy) + sz * sz;
            const bool usable = __ballot(!sane) == 0ull && len2 >= 1e-6f && len2 <= 4.0f;
            if (!usable) {                                       // (uniform: every lane holds the same sums)
                if (lane < kCpCone) rec[lane] = 0.0f;
                return;
            }
            const float il = 1.0f / __builtin_sqrtf(len2);
            ax = sx * il; ay = sy * il; az = sz * il;
        }
    }
    float least = cb;
    for (int d = 32; d > 0; d >>= 1) least = __builtin_fminf(least, __shfl_xor(least, d, 64));
    least = __shfl(least, 0, 64);
    const unsigned long long who = __ballot(cb == least);
    const float sine = __shfl(sb, who ? __ffsll((long long)who) - 1 : 0, 64);
    if (lane == 0) {
        rec[0] = ax; rec[1] = ay; rec[2] = az; rec[3] = least; rec[4] = sine;
        rec[5] = least <= 1.5f ? 1.0f : 0.0f;                    // (no lane saw a point: the tables disagree, not usable)
        rec[6] = lo; rec[7] = hi;
    }
}

// ------------------------------------------------------------------------------------------- k nearest points, normals
// A lane's list: k keys in LDS, slot j of lane t at list[j * lanes + t] (the lanes of a wavefront are contiguous, so
// every ds_read_b64 / ds_write_b64 is free of bank conflicts, whatever slot each lane is at: a row of slots is a multiple
// of 256 bytes).  While the walk runs `n` slots are filled, in arrival order until n == k; from then on the k slots are
// a binary max-heap (children of slot i at 2 i + 1 and 2 i + 2) whose root is `root`, the lane's k-th key so far.
// Until then root is (limit bits, -1), above every admissible key.  It is the other sink of pc_walk.
struct PcList {
    unsigned long long* at;      // the lane's slot 0
    int lanes, k, n;
    float limit;
    unsigned long long root;
    __device__ __forceinline__ unsigned long long bound() const { return root; }
    __device__ __forceinline__ void offer(float d2, unsigned long long key);
    __device__ __forceinline__ bool skip_block(long long) const { return false; }
};

// v into slot i of the max-heap of the first n slots: the larger child moves up until v is no smaller than both
static __device__ __forceinline__ void pc_list_sift(unsigned long long* at, int lanes, int n, int i, unsigned long long v)
{
    for (;;) {
        int c = 2 * i + 1;
        if (c >= n) break;
        unsigned long long a = at[(size_t)c * lanes];
        if (c + 1 < n) {
            const unsigned long long b = at[(size_t)(c + 1) * lanes];
            if (b > a) { a = b; ++c; }
        }
        if (a <= v) break;
        at[(size_t)i * lanes] = a;
        i = c;
    }
    at[(size_t)i * lanes] = v;
}

__device__ __forceinline__ void PcList::offer(float d2, unsigned long long key)
{
    if (!(d2 <= limit) || key >= root) return;
    if (n < k) {
        at[(size_t)n * lanes] = key;
        if (++n < k) return;                                   // not full: the bound stays at limit
        for (int i = k / 2 - 1; i >= 0; --i) pc_list_sift(at, lanes, k, i, at[(size_t)i * lanes]);
    } else {
        pc_list_sift(at, lanes, k, 0, key);                     // in place of the maximum
    }
    root = at[0];
}

// the n keys of the list in ascending order, in place (heap sort: the root goes behind the shrinking heap)
static __device__ __forceinline__ void pc_list_sort(PcList& l)
{
    if (l.n < l.k)
        for (int i = l.n / 2 - 1; i >= 0; --i) pc_list_sift(l.at, l.lanes, l.n, i, l.at[(size_t)i * l.lanes]);
    for (int end = l.n - 1; end > 0; --end) {
        const unsigned long long v = l.at[(size_t)end * l.lanes];
        l.at[(size_t)end * l.lanes] = l.at[0];
        pc_list_sift(l.at, l.lanes, end, 0, v);
    }
}

// The whole k-nearest query of lane `lane` of the workgroup for entry i of body b: the query, the search, the sort.
// Returns n; the lane's slots 0 .. n - 1 then hold its keys in ascending order.  (qx, qy, qz) is the query where n > 0.
static __device__ __forceinline__ int pc_knn_lane(const PcTables& w, const float* __restrict__ queries,
                                                  const float* __restrict__ shift, const int32_t* __restrict__ query_counts,
                                                  float limit, int b, int Q, int N, int i, int k, unsigned long long* list,
                                                  int lanes, int lane, float& qx, float& qy, float& qz)
{
    if (i >= pc_entries(query_counts, b, N)) return 0;
    pc_entry(queries, shift, b, N, i, qx, qy, qz);
    if (!pc_finite3(qx, qy, qz)) return 0;
    PcList l;
    l.at = list + lane;
    l.lanes = lanes; l.k = k; l.n = 0;
    l.limit = limit;
    l.root = pc_key(limit, -1);
    l = pc_walk(w, b, Q, qx, qy, qz, l);                      // the n <= k smallest admissible keys, unsorted
    pc_list_sort(l);
    return l.n;
}

// blockDim.x lanes (a multiple of 64), k * blockDim.x keys of dynamic LDS
__global__ __launch_bounds__(kBlock) void pc_knn_kernel(PcTables w, const float* __restrict__ queries,
                                                       const float* __restrict__ shift,
                                                       const int32_t* __restrict__ query_counts, float limit, int Q, int N,
                                                       int k, float* __restrict__ d2_out, int32_t* __restrict__ index_out)
{
    extern __shared__ unsigned long long pc_keys[];
    const int lanes = blockDim.x, lane = threadIdx.x;
    const int b = blockIdx.y, i = blockIdx.x * lanes + lane;
    if (i >= N) return;
    float qx, qy, qz;
    const int n = pc_knn_lane(w, queries, shift, query_counts, limit, b, Q, N, i, k, pc_keys, lanes, lane, qx, qy, qz);
    const size_t o = ((size_t)b * N + i) * k;
    for (int j = 0; j < k; ++j) {                               // (a slot below n holds a point's key; kPcNoKey is +inf, -1)
        const unsigned long long key = j < n ? pc_keys[(size_t)j * lanes + lane] : kPcNoKey;
        d2_out[o + j] = pc_key_d2(key);
        index_out[o + j] = pc_key_index(key);
    }
}

// The normal of a neighbourhood.  C is the float32 scatter matrix of the rule, T = trace C + n |m|^2 = sum_j |d_j|^2.
//
// The error bound E = c u T, u = 2^-24, c = n + kPcSolverC, against the float64 scatter matrix of the same neighbours
// (the SAME float32 points and query, every operation exact).  Write d, m, e, C for the exact values.
//   The differences: fl(d_j) = d_j + a_j, |a_j| <= u |d_j| per component.  The mean: fl(m) = m + h with
// |h| <= (n + 1) u mean|d| (n - 1 additions, the a_j, one division).  The centred rows: fl(e_j) = e_j + a_j - h + r_j,
// |r_j| <= u |e_j|.  In sum_j fl(e_j) fl(e_j)^T the first-order share of h is -(sum_j e_j) h^T - h (sum_j e_j)^T = 0
// EXACTLY, because the e_j sum to zero: the mean's error enters only as n h h^T, of norm <= (n + 1)^2 u^2 T < 0.001 u T
// for n <= 32.  The first-order share of a and r is sum_j e_j (a_j + r_j)^T + its transpose, of Frobenius norm
//     <= 2 u sum_j |e_j| (|d_j| + |e_j|)  <=  2 u (sqrt(trace C  T) + trace C)  <=  4 u T      (Cauchy-Schwarz, trace C <= T).
// Each entry's sum: one rounding per product and n - 1 per left-to-right sum, n u sum_j |e_j,a e_j,b| <= n u sqrt(C_aa C_bb),
// a matrix of Frobenius norm n u trace C <= n u T.  Together || fl(C) - C ||_F <= (n + 4.01) u T.
//   The solver: kPcSweeps cyclic sweeps (0,1), (0,2), (1,2) of Jacobi rotations, t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)),
// c = 1 / sqrt(t^2 + 1), s = t c, no branch and no trigonometric call.  A computed rotation is the exact similarity of
// a matrix 14 u ||A||_F away (t with 5 u relative error, which leaves 5 u |apq| where the update writes 0 and as much on
// the two diagonal entries; c^2 + s^2 = 1 within 5 u; three operations per updated entry), ||A||_F <= trace C (1 + O(u))
// throughout: 3 kPcSweeps 14 u = 210 u T for the 15 rotations.  What the
// last sweep leaves off the diagonal is a perturbation of its own: rows whose residual sqrt(2 (a01^2 + a02^2 + a12^2))
// exceeds u T are given up (a zero normal) -- quadratic convergence leaves none on any input tried -- so it adds 1 u T.
// The vector itself: 15 updates of V at 3 u each and the normalisation, < 50 u of angle, not amplified by any gap; it is
// counted as 25 u T in E because the angle bound below is 2 E / gap >= 2 E / T.  210 + 4.01 + 1 + 25 < kPcSolverC = 256
// (the rest covers T's own rounding and second-order terms).
//   By Weyl every eigenvalue is within E of the exact one; by Davis-Kahan (in the form sin <= 2 ||D|| / gap, the gap that
// of the EXACT matrix) the sine of the angle between the computed and the exact normal is at most 2 E / (lambda1 -
// lambda0).  The normal is a zero row where that says nothing: n < 3, 2 E >= lambda1 - lambda0 as computed, a
// residual above u T, or T below kPcNormal (products without relative accuracy) or not finite.  variation = lambda0 /
// (lambda0 + lambda1 + lambda2) is then within 2 E / trace C + 2 u of the float64 value (three eigenvalue errors in the
// denominator weighted by lambda0 / trace <= 1 / 3, one in the numerator, the sum's and the division's roundings).
constexpr int kPcSweeps = 5;
constexpr float kPcSolverC = 256.0f;
constexpr float kPcU = 5.9604644775390625e-8f;          // u = 2^-24

// One Jacobi rotation in the (p, q) plane; r is the third index.  arp = A[r][p], arq = A[r][q]; vp, vq: columns p, q of V.
static __device__ __forceinline__ void pc_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float (&vp)[3],
                                                 float (&vq)[3])
{
    const float theta = (aqq - app) / (2.0f * apq);
    float t = __builtin_copysignf(1.0f, theta) / (__builtin_fabsf(theta) + __builtin_sqrtf(theta * theta + 1.0f));
    t = (apq != 0.0f && __builtin_isfinite(t)) ? t : 0.0f;    // (theta overflowing: the rotation is the identity)
    const float c = 1.0f / __builtin_sqrtf(t * t + 1.0f), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = t != 0.0f ? 0.0f : apq;
    const float np = c * arp - s * arq, nq = s * arp + c * arq;
    arp = np; arq = nq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = c * vp[r] - s * vq[r], d = s * vp[r] + c * vq[r];
        vp[r] = a; vq[r] = d;
    }
}

__global__ __launch_bounds__(kBlock) void pc_normals_kernel(PcTables w, const float* __restrict__ points,
                                                           const float* __restrict__ queries,
                                                           const float* __restrict__ shift,
                                                           const int32_t* __restrict__ query_counts, float limit, int Q, int N,
                                                           int k, const float* __restrict__ viewpoint, int view_layout,
                                                           float* __restrict__ normal_out, float* __restrict__ variation_out,
                                                           int32_t* __restrict__ count_out, float* __restrict__ cov_out)
{
    extern __shared__ unsigned long long pc_keys[];
    const int lanes = blockDim.x, lane = threadIdx.x;
    const int b = blockIdx.y, i = blockIdx.x * lanes + lane;
    if (i >= N) return;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    const int n = pc_knn_lane(w, queries, shift, query_counts, limit, b, Q, N, i, k, pc_keys, lanes, lane, qx, qy, qz);
    const float* body = points + (size_t)b * Q * 3;
    // the mean of d_j = s_j - q, in key order
    float mx = 0.0f, my = 0.0f, mz = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float* s = body + (size_t)pc_clampi(pc_key_index(pc_keys[(size_t)j * lanes + lane]), 0, Q - 1) * 3;
        const float dx = pc_sub(s[0], qx), dy = pc_sub(s[1], qy), dz = pc_sub(s[2], qz);
        mx = j == 0 ? dx : pc_add(mx, dx); my = j == 0 ? dy : pc_add(my, dy); mz = j == 0 ? dz : pc_add(mz, dz);
    }
    if (n > 0) { mx = mx / (float)n; my = my / (float)n; mz = mz / (float)n; }
    float cxx = 0.0f, cxy = 0.0f, cxz = 0.0f, cyy = 0.0f, cyz = 0.0f, czz = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float* s = body + (size_t)pc_clampi(pc_key_index(pc_keys[(size_t)j * lanes + lane]), 0, Q - 1) * 3;
        const float ex = pc_sub(pc_sub(s[0], qx), mx), ey = pc_sub(pc_sub(s[1], qy), my), ez = pc_sub(pc_sub(s[2], qz), mz);
        cxx = pc_add(cxx, pc_mul(ex, ex)); cxy = pc_add(cxy, pc_mul(ex, ey)); cxz = pc_add(cxz, pc_mul(ex, ez));
        cyy = pc_add(cyy, pc_mul(ey, ey)); cyz = pc_add(cyz, pc_mul(ey, ez)); czz = pc_add(czz, pc_mul(ez, ez));
    }
    const size_t o = (size_t)b * N + i;
    if (cov_out) {
        float* c = cov_out + o * 6;
        c[0] = cxx; c[1] = cxy; c[2] = cxz; c[3] = cyy; c[4] = cyz; c[5] = czz;
    }
    const float total = pc_add(pc_add(pc_add(cxx, cyy), czz),
                               pc_mul((float)n, pc_add(pc_add(pc_mul(mx, mx), pc_mul(my, my)), pc_mul(mz, mz))));
    const float err = pc_mul(pc_mul((float)n + kPcSolverC, kPcU), total);          // E
    float a00 = cxx, a01 = cxy, a02 = cxz, a11 = cyy, a12 = cyz, a22 = czz;
    float v0[3] = {1.0f, 0.0f, 0.0f}, v1[3] = {0.0f, 1.0f, 0.0f}, v2[3] = {0.0f, 0.0f, 1.0f};
#pragma unroll
    for (int sweep = 0; sweep < kPcSweeps; ++sweep) {
        pc_rotate(a00, a11, a01, a02, a12, v0, v1);
        pc_rotate(a00, a22, a02, a01, a12, v0, v2);
        pc_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    const float residual = __builtin_sqrtf(2.0f * ((a01 * a01 + a02 * a02) + a12 * a12));
    // the smallest eigenvalue's column, the two smallest eigenvalues
    const bool first = a00 <= a11 && a00 <= a22, second = !first && a11 <= a22;
    const float l0 = first ? a00 : (second ? a11 : a22);
    const float l1 = first ? __builtin_fminf(a11, a22) : (second ? __builtin_fminf(a00, a22) : __builtin_fminf(a00, a11));
    const float l2 = first ? __builtin_fmaxf(a11, a22) : (second ? __builtin_fmaxf(a00, a22) : __builtin_fmaxf(a00, a11));
    float nx = first ? v0[0] : (second ? v1[0] : v2[0]), ny = first ? v0[1] : (second ? v1[1] : v2[1]),
          nz = first ? v0[2] : (second ? v1[2] : v2[2]);
    const float len = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
    const bool known = n >= 3 && total >= kPcNormal && total <= kPcMaxD2 && 2.0f * err < l1 - l0 &&
                       residual <= kPcU * total && len > 0.5f;
    float variation = 0.0f;
    if (known) {
        nx = nx / len; ny = ny / len; nz = nz / len;
        // canonical sign: the component of the largest magnitude is positive, the first among equals
        const float ax = __builtin_fabsf(nx), ay = __builtin_fabsf(ny), az = __builtin_fabsf(nz);
        const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
        bool flip = lead < 0.0f;
        if (view_layout != 0) {
            const float* c = viewpoint + (view_layout == 2 ? o : (size_t)b) * 3;
            const float sx = flip ? -nx : nx, sy = flip ? -ny : ny, sz = flip ? -nz : nz;
            const float side = pc_add(pc_add(pc_mul(sx, pc_sub(c[0], qx)), pc_mul(sy, pc_sub(c[1], qy))),
                                      pc_mul(sz, pc_sub(c[2], qz)));
            if (side < 0.0f) flip = !flip;
        }
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        const float low = __builtin_fmaxf(l0, 0.0f);
        variation = low / ((low + l1) + l2);
    } else {
        nx = 0.0f; ny = 0.0f; nz = 0.0f;
    }
    normal_out[o * 3] = nx; normal_out[o * 3 + 1] = ny; normal_out[o * 3 + 2] = nz;
    variation_out[o] = variation;
    count_out[o] = n;
}

// ---------------------------------------------------------------------------------------------------------- the term
#pragma clang fp contract(fast)

// vertex weights: layout 0 none (ones), 1 [V], 2 [B,V]
static __device__ __forceinline__ float pc_weight(const float* __restrict__ vw, int layout, int b, int V, int v)
{
    return layout == 0 ? 1.0f : vw[(layout == 2 ? (size_t)b * V : (size_t)0) + v];
}

// the mesh of the oriented term: the lane that owns a vertex forms its normal itself (face_normal.h: vn_vertex_normal)
struct PcMesh {
    const int32_t* faces;        // [F][3]
    const int32_t* vf_off;       // [V + 1]
    const int32_t* vf_ids;       // [3 F]
    int F;
};

// The term (tuch_point_cloud_fit_terms; kOriented: with normals).  kOriented: the query is the oriented one, with
// the raw vertex normal of the UNTRANSLATED verts (tuch_vertex_normals' row, normalize = 0); nothing else differs, and
// the plain form reads neither orient nor mesh.  (The arguments stay a list: as one struct by value they are all loaded
// at entry, and this kernel, which is at its SGPR limit, then spills them to VGPR lanes and reloads them inside the
// walk -- 81 v_readlane against 19, docs/HISTORY.md section 13.)
template <bool kOriented>
__global__ __launch_bounds__(kBlock) void pc_fit_kernel(PcTables w, PcOrient orient, PcMesh mesh,
                                                       const float* __restrict__ points,
                                                       const int32_t* __restrict__ counts, const float* __restrict__ weights,
                                                       const float* __restrict__ verts, const float* __restrict__ transl,
                                                       const int32_t* hint, float limit, int has_tau, int B, int Q, int V,
                                                       const float* __restrict__ vw, int layout, int rho, float sigma2,
                                                       float scale, float* __restrict__ d2_out, int32_t* index_out,
                                                       float* partial, int* ticket, float* __restrict__ per_body,
                                                       float* __restrict__ total, float* __restrict__ grad_verts,
                                                       float* __restrict__ grad_transl)
{
    __shared__ FitShared sh;
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    // the normaliser: this body's vertex weights
    float wsum = (float)V;
    if (layout != 0) wsum = fit_body_sum(sh, V, [&](int i) { return pc_weight(vw, layout, b, V, i); });
    const int cloud = pc_clampi((int)w.head[kCtl + (size_t)b * kHead + H_N], 0, Q);
    const int v = c * kBlock + t;
    float s = 0.0f, ex = 0.0f, ey = 0.0f, ez = 0.0f;
    if (v < V) {
        const size_t o = (size_t)b * V + v;
        const float wv = pc_weight(vw, layout, b, V, v);
        unsigned long long best = kPcNoKey;
        float qx = 0.0f, qy = 0.0f, qz = 0.0f;
        const bool live = wv != 0.0f && wsum != 0.0f && cloud > 0;
        const int h = hint ? hint[o] : -1;
        if (live) {
            pc_entry<true>(verts, transl, b, V, v, qx, qy, qz);
            float ux = 0.0f, uy = 0.0f, uz = 0.0f;
            if constexpr (kOriented)
                vn_vertex_normal(verts + (size_t)b * V * 3, mesh.faces, mesh.vf_off, mesh.vf_ids, V, mesh.F, v, ux, uy, uz);
            best = pc_query<kOriented>(w, orient, points, counts, weights, b, Q, qx, qy, qz, ux, uy, uz, h, limit);
        }
        const bool won = pc_won(best);
        const float d2 = won ? pc_key_d2(best) : __builtin_inff();
        const int idx = won ? pc_key_index(best) : -1;
        d2_out[o] = d2;
        index_out[o] = idx;
        if (won) {
            float value, slope;
            fit_rho(rho, sigma2, d2, value, slope);
            s = wv * value;
            const float g2 = 2.0f * (scale * wv * slope / wsum);
            const float* p = points + ((size_t)b * Q + pc_clampi(idx, 0, Q - 1)) * 3;
            ex = g2 * (qx - p[0]); ey = g2 * (qy - p[1]); ez = g2 * (qz - p[2]);
        } else if (live && has_tau) {
            float value, slope;
            fit_rho(rho, sigma2, limit, value, slope);
            s = wv * value;
        }
        float* gv = grad_verts + o * 3;
        gv[0] = ex; gv[1] = ey; gv[2] = ez;
    }
    fit_reduce_tail(sh, s, ex, ey, ez, wsum, scale, partial, ticket, B, per_body, total, grad_transl);
}

bool pc_sizes_ok(int B, int Q, int N)
{
    return B > 0 && B <= 65535 && Q > 0 && N > 0 && (long long)B * Q < (1ll << 31) && (long long)B * N < (1ll << 31) &&
           (long long)B * ceil_div(N, kBlock) < (1ll << 30);
}

PcTables pc_tables(void* workspace, size_t bytes, int B, int Q)
{
    const PcLayout l = pc_layout(B, Q, 0);
    PcTables w;
    w.head = (const uint32_t*)((char*)workspace + l.head);
    w.sorted = (const float4*)((char*)workspace + l.sorted);
    w.tables = (const int32_t*)((char*)workspace + l.tables);
    w.cap = (long long)((bytes - l.tables) / sizeof(int32_t));
    return w;
}

// the limit of a query: f32(tau) f32(tau), or the largest finite d2 (max_distance <= 0: none)
float pc_limit(float max_distance) { return max_distance > 0.0f ? fminf(max_distance * max_distance, kPcMaxD2) : kPcMaxD2; }

// Every entry point that queries: the workspace holds the regions a query addresses by themselves, the term's scratch
// (scratch_need != 0) its partials.  Called inside the entry point's tuch_ws_scope, which stays alive up to the launch:
// the layout, like pc_tables' after it, is the guarded one under the canary option.
int pc_workspace_check(const char* name, size_t workspace_bytes, int B, int Q, size_t scratch_bytes = 0, size_t scratch_need = 0)
{
    const size_t need = pc_layout(B, Q, 1).total;
    if (workspace_bytes >= need && scratch_bytes >= scratch_need) return TUCH_OK;
    if (scratch_need)
        tuch_set_error("%s: workspace %zu < %zu or scratch %zu < %zu bytes", name, workspace_bytes, need, scratch_bytes,
                       scratch_need);
    else
        tuch_set_error("%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
    return TUCH_ERR_WORKSPACE;
}

size_t pc_cone_words(int B, int R)
{
    const size_t c = (size_t)((R + 3) >> 2);
    return (size_t)kCpCone + (size_t)B * c * c * c * kCpCone;
}

// what the oriented launches take; cones NULL: none
PcOrient pc_orient(const float* normals, float max_angle_cos, const void* cones, size_t cones_bytes)
{
    PcOrient o;
    o.normals = normals;
    o.cones = (const uint32_t*)cones;
    o.cone_cap = cones && cones_bytes >= 2 * kCpCone * sizeof(float) ? (long long)(cones_bytes / (kCpCone * sizeof(float))) - 1 : 0;
    if (o.cone_cap == 0) o.cones = nullptr;
    o.c = fminf(fmaxf(max_angle_cos, 0.0f), 1.0f);
    o.c2 = o.c * o.c;
    return o;
}

}  // namespace

// the query and the term: normals == nullptr is the plain form of each
extern "C" int tuch_point_cloud_nearest(const void* workspace, size_t workspace_bytes, const float* points,
                                        const int32_t* counts, const float* weights, const float* normals,
                                        const float* queries, const float* query_normals, const float* shift,
                                        const int32_t* query_counts, const int32_t* hint, float max_distance,
                                        float max_angle_cos, const void* cones, size_t cones_bytes, int B, int Q, int N,
                                        float* d2, int32_t* index, void* stream)
{
    const char* name = "tuch_point_cloud_nearest";
    TUCH_REQUIRE(!normals == !query_normals, "%s: normals and query_normals go together (%p, %p)", name, (const void*)normals,
                 (const void*)query_normals);
    const bool oriented = normals != nullptr;
    TUCH_REQUIRE(!oriented || (max_angle_cos >= 0.0f && max_angle_cos < 1.0f), "%s: max_angle_cos %g (in [0, 1))", name,
                 (double)max_angle_cos);
    TUCH_REQUIRE(workspace && points && queries && d2 && index, "%s: null pointer", name);
    TUCH_REQUIRE(pc_sizes_ok(B, Q, N), "%s: bad sizes B=%d Q=%d N=%d", name, B, Q, N);
    tuch_ws_scope scope(g_pc_canary != 0);
    const int rc = pc_workspace_check(name, workspace_bytes, B, Q);
    if (rc != TUCH_OK) return rc;
    // (not oriented: the cosine and the cones are not read)
    const PcOrient orient = oriented ? pc_orient(normals, max_angle_cos, cones, cones_bytes) : pc_orient(nullptr, 0.0f, nullptr, 0);
    hipLaunchKernelGGL(oriented ? pc_nearest_kernel<true> : pc_nearest_kernel<false>, dim3(ceil_div(N, kBlock), B), dim3(kBlock), 0,
                       (hipStream_t)stream, pc_tables((void*)workspace, workspace_bytes, B, Q), orient, points, counts, weights,
                       queries, query_normals, shift, query_counts, hint, pc_limit(max_distance), Q, N, d2, index);
    return tuch_check_launch(name);
}

extern "C" int tuch_point_cloud_fit_terms(const void* workspace, size_t workspace_bytes, const float* points,
                                          const int32_t* counts, const float* weights, const float* normals,
                                          float max_angle_cos, const int32_t* faces, const int32_t* vf_off,
                                          const int32_t* vf_ids, int F, const void* cones, size_t cones_bytes,
                                          const float* verts, const float* transl, const int32_t* hint, float max_distance,
                                          int B, int Q, int V, const float* vertex_weights, int vertex_weight_layout, int rho,
                                          float sigma, float scale, float* d2, int32_t* index, int* ticket, float* per_body,
                                          float* total, float* grad_verts, float* grad_transl, void* scratch,
                                          size_t scratch_bytes, void* stream)
{
    const char* name = "tuch_point_cloud_fit_terms";
    const bool oriented = normals != nullptr;
    if (oriented) {
        TUCH_REQUIRE(faces && vf_off && vf_ids, "%s: null pointer", name);
        TUCH_REQUIRE(pc_sizes_ok(B, Q, V) && F > 0 && (long long)F * 3 < (1ll << 31), "%s: bad sizes B=%d Q=%d V=%d F=%d", name, B,
                     Q, V, F);
        TUCH_REQUIRE(max_angle_cos >= 0.0f && max_angle_cos < 1.0f, "%s: max_angle_cos %g (in [0, 1))", name,
                     (double)max_angle_cos);
    }
    TUCH_REQUIRE(workspace && points && verts && transl && d2 && index && ticket && per_body && total && grad_verts &&
                     grad_transl && scratch,
                 "%s: null pointer", name);
    TUCH_REQUIRE(pc_sizes_ok(B, Q, V), "%s: bad sizes B=%d Q=%d V=%d", name, B, Q, V);
    TUCH_REQUIRE(vertex_weight_layout >= 0 && vertex_weight_layout <= 2 && (vertex_weight_layout == 0 || vertex_weights),
                 "%s: vertex weight layout %d (0 none, 1 [V], 2 [B,V]) with weights %p", name, vertex_weight_layout,
                 (const void*)vertex_weights);
    TUCH_REQUIRE(rho == TUCH_SCAN_RHO_SQUARED || rho == TUCH_SCAN_RHO_DISTANCE || (rho == TUCH_SCAN_RHO_GMOF && sigma > 0.0f),
                 "%s: rho %d (0 squared, 1 distance, 2 gmof with sigma > 0; sigma = %g)", name, rho, (double)sigma);
    tuch_ws_scope scope(g_pc_canary != 0);
    const PcScratch sl = scope.record(0, [&] { return pc_scratch(B, V); });
    const int rc = pc_workspace_check(name, workspace_bytes, B, Q, scratch_bytes, sl.total);
    if (rc != TUCH_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const PcTables w = pc_tables((void*)workspace, workspace_bytes, B, Q);
    scope.arm(scratch, (int32_t*)w.head, s);
    // (not oriented: no mesh, no cones, and the cosine is not read)
    const PcOrient orient = oriented ? pc_orient(normals, max_angle_cos, cones, cones_bytes) : pc_orient(nullptr, 0.0f, nullptr, 0);
    const PcMesh mesh = oriented ? PcMesh{faces, vf_off, vf_ids, F} : PcMesh{};
    hipLaunchKernelGGL(oriented ? pc_fit_kernel<true> : pc_fit_kernel<false>, dim3(ceil_div(V, kBlock), B), dim3(kBlock), 0, s, w,
                       orient, mesh, points, counts, weights, verts, transl, hint, pc_limit(max_distance),
                       max_distance > 0.0f ? 1 : 0, B, Q, V, vertex_weights, vertex_weight_layout, rho, sigma * sigma, scale, d2,
                       index, (float*)((char*)scratch + sl.partial), ticket, per_body, total, grad_verts, grad_transl);
    return tuch_check_launch(name);
}

extern "C" int tuch_point_cloud_set_canary(int on)
{
    const int was = g_pc_canary;
    g_pc_canary = on != 0;
    return was;
}

extern "C" size_t tuch_point_cloud_workspace_bytes(int B, int Q, int resolution)
{
    if (B <= 0 || Q <= 0 || resolution <= 0 || resolution > kMaxRes) return 0;
    tuch_ws_scope scope(g_pc_canary != 0);
    return pc_layout(B, Q, resolution).total;
}

extern "C" size_t tuch_point_cloud_fit_scratch_bytes(int B, int N)
{
    if (B <= 0 || N <= 0) return 0;
    tuch_ws_scope scope(g_pc_canary != 0);
    return pc_scratch(B, N).total;
}

extern "C" int tuch_point_cloud_build(const float* points, const int32_t* counts, const float* weights, int B, int Q,
                                      int resolution, void* workspace, size_t workspace_bytes, void* stream)
{
    TUCH_REQUIRE(points && workspace, "tuch_point_cloud_build: null pointer");
    TUCH_REQUIRE(pc_sizes_ok(B, Q, 1) && resolution > 0 && resolution <= kMaxRes,
                 "tuch_point_cloud_build: bad sizes B=%d Q=%d resolution=%d (1 .. %d)", B, Q, resolution, kMaxRes);
    const size_t need = tuch_point_cloud_workspace_bytes(B, Q, resolution);
    if (workspace_bytes < need) {
        tuch_set_error("tuch_point_cloud_build: workspace %zu < %zu bytes", workspace_bytes, need);
        return TUCH_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    tuch_ws_scope scope(g_pc_canary != 0);
    const PcLayout l = scope.record(0, [&] { return pc_layout(B, Q, resolution); });
    uint32_t* head = (uint32_t*)((char*)workspace + l.head);
    scope.arm(workspace, (int32_t*)head, s);
    float4* sorted = (float4*)((char*)workspace + l.sorted);
    int32_t* tables = (int32_t*)((char*)workspace + l.tables);
    const size_t ints = (size_t)B * pc_table_ints(resolution);
    TUCH_REQUIRE((ints + kBlock - 1) / kBlock < (1ull << 31), "tuch_point_cloud_build: tables too large (B=%d resolution=%d)", B,
                 resolution);
    tuch_launch_zero_words(tables, ints, s);
    hipLaunchKernelGGL(pc_header_kernel, dim3(B), dim3(kBlock), 0, s, points, counts, weights, Q, resolution, head);
    const dim3 grid(ceil_div(Q, kBlock), B);
    hipLaunchKernelGGL(pc_file_kernel<false>, grid, dim3(kBlock), 0, s, points, counts, weights, Q, resolution,
                       (const uint32_t*)head, tables, sorted);
    hipLaunchKernelGGL(pc_scan_kernel, dim3(B), dim3(kBlock), 0, s, (const uint32_t*)head, resolution, tables);
    hipLaunchKernelGGL(pc_file_kernel<true>, grid, dim3(kBlock), 0, s, points, counts, weights, Q, resolution,
                       (const uint32_t*)head, tables, sorted);
    return tuch_check_launch("tuch_point_cloud_build");
}

namespace {

// Lanes per workgroup of the k-nearest kernels: 256 up to k = 16, 128 beyond, so a workgroup's list (k x lanes x 8
// bytes) never exceeds 32 KiB and five workgroups fit into a CU's 160 KiB of LDS -- 20 wavefronts at k <= 16, 10 beyond.
int pc_knn_lanes(int k) { return k > 16 ? kBlock / 2 : kBlock; }

int pc_knn_check(const char* name, size_t workspace_bytes, int B, int Q, int N, int k)
{
    TUCH_REQUIRE(pc_sizes_ok(B, Q, N) && (long long)B * N * k < (1ll << 31), "%s: bad sizes B=%d Q=%d N=%d k=%d", name, B, Q, N,
                 k);
    return pc_workspace_check(name, workspace_bytes, B, Q);
}

}  // namespace

extern "C" int tuch_point_cloud_knn(const void* workspace, size_t workspace_bytes, const float* points, const int32_t* counts,
                                    const float* weights, const float* queries, const float* shift,
                                    const int32_t* query_counts, float max_distance, int B, int Q, int N, int k, float* d2,
                                    int32_t* index, void* stream)
{
    TUCH_REQUIRE(workspace && points && queries && d2 && index, "tuch_point_cloud_knn: null pointer");
    TUCH_REQUIRE(k >= 1 && k <= 32, "tuch_point_cloud_knn: k = %d (1 .. 32)", k);
    tuch_ws_scope scope(g_pc_canary != 0);                     // alive up to the launch: pc_tables lays the regions out in it
    const int rc = pc_knn_check("tuch_point_cloud_knn", workspace_bytes, B, Q, N, k);
    if (rc != TUCH_OK) return rc;
    (void)counts; (void)weights;        // (the build filed the valid points; the ABI keeps the triple together)
    const int lanes = pc_knn_lanes(k);
    hipLaunchKernelGGL(pc_knn_kernel, dim3(ceil_div(N, lanes), B), dim3(lanes), (size_t)k * lanes * sizeof(unsigned long long),
                       (hipStream_t)stream, pc_tables((void*)workspace, workspace_bytes, B, Q), queries, shift, query_counts,
                       pc_limit(max_distance), Q, N, k, d2, index);
    return tuch_check_launch("tuch_point_cloud_knn");
}

extern "C" int tuch_point_cloud_normals(const void* workspace, size_t workspace_bytes, const float* points,
                                        const int32_t* counts, const float* weights, const float* queries, const float* shift,
                                        const int32_t* query_counts, float max_distance, int B, int Q, int N, int k,
                                        const float* viewpoint, int viewpoint_layout, float* normals, float* variation,
                                        int32_t* count, float* cov, void* stream)
{
    TUCH_REQUIRE(workspace && points && queries && normals && variation && count, "tuch_point_cloud_normals: null pointer");
    TUCH_REQUIRE(k >= 1 && k <= 32, "tuch_point_cloud_normals: k = %d (1 .. 32)", k);
    TUCH_REQUIRE(viewpoint_layout >= 0 && viewpoint_layout <= 2 && (viewpoint_layout == 0 || viewpoint),
                 "tuch_point_cloud_normals: viewpoint layout %d (0 none, 1 [B,3], 2 [B,N,3]) with viewpoint %p", viewpoint_layout,
                 (const void*)viewpoint);
    tuch_ws_scope scope(g_pc_canary != 0);
    const int rc = pc_knn_check("tuch_point_cloud_normals", workspace_bytes, B, Q, N, k);
    if (rc != TUCH_OK) return rc;
    (void)counts; (void)weights;
    const int lanes = pc_knn_lanes(k);
    hipLaunchKernelGGL(pc_normals_kernel, dim3(ceil_div(N, lanes), B), dim3(lanes),
                       (size_t)k * lanes * sizeof(unsigned long long), (hipStream_t)stream,
                       pc_tables((void*)workspace, workspace_bytes, B, Q), points, queries, shift, query_counts,
                       pc_limit(max_distance), Q, N, k, viewpoint, viewpoint_layout, normals, variation, count, cov);
    return tuch_check_launch("tuch_point_cloud_normals");
}

// -------------------------------------------------------------------------------------------------------- the cones
extern "C" size_t tuch_point_cloud_cones_bytes(int B, int resolution)
{
    if (B <= 0 || resolution <= 0 || resolution > kMaxRes) return 0;
    return pc_cone_words(B, resolution) * sizeof(float);
}

extern "C" int tuch_point_cloud_build_cones(const void* workspace, size_t workspace_bytes, const float* normals, int B, int Q,
                                            int resolution, void* cones, size_t cones_bytes, void* stream)
{
    TUCH_REQUIRE(workspace && normals && cones, "tuch_point_cloud_build_cones: null pointer");
    TUCH_REQUIRE(pc_sizes_ok(B, Q, 1) && resolution > 0 && resolution <= kMaxRes,
                 "tuch_point_cloud_build_cones: bad sizes B=%d Q=%d resolution=%d (1 .. %d)", B, Q, resolution, kMaxRes);
    tuch_ws_scope scope(g_pc_canary != 0);
    const size_t need = pc_layout(B, Q, resolution).total, cone_need = tuch_point_cloud_cones_bytes(B, resolution);
    if (workspace_bytes < need || cones_bytes < cone_need) {
        tuch_set_error("tuch_point_cloud_build_cones: workspace %zu < %zu or cones %zu < %zu bytes", workspace_bytes, need,
                       cones_bytes, cone_need);
        return TUCH_ERR_WORKSPACE;
    }
    const int cres = (resolution + 3) >> 2;
    hipLaunchKernelGGL(pc_cones_kernel, dim3(cres * cres * cres, B), dim3(64), 0, (hipStream_t)stream,
                       pc_tables((void*)workspace, workspace_bytes, B, Q), normals, Q, resolution, (uint32_t*)cones);
    return tuch_check_launch("tuch_point_cloud_build_cones");
}

extern "C" int tuch_point_cloud_grid(const void* workspace, int B, int resolution, float* origin_host, float* cell_host,
                                     int32_t* dims_host)
{
    TUCH_REQUIRE(workspace && origin_host && cell_host && dims_host, "tuch_point_cloud_grid: null pointer");
    TUCH_REQUIRE(B > 0 && B <= 65535 && resolution > 0 && resolution <= kMaxRes,
                 "tuch_point_cloud_grid: bad sizes B=%d resolution=%d", B, resolution);
    std::vector<uint32_t> head((size_t)B * kHead);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(head.data(), (const uint32_t*)workspace + kCtl, head.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) !=
            hipSuccess) {
        tuch_set_error("tuch_point_cloud_grid: %s", hipGetErrorString(hipGetLastError()));
        return TUCH_ERR_HIP;
    }
    for (int b = 0; b < B; ++b) {
        const uint32_t* h = head.data() + (size_t)b * kHead;
        for (int k = 0; k < 3; ++k) {
            memcpy(origin_host + 3 * b + k, h + H_OX + k, sizeof(float));
            dims_host[3 * b + k] = (int32_t)h[H_DX + k];
        }
        memcpy(cell_host + b, h + H_CELL, sizeof(float));
    }
    return TUCH_OK;
}

extern "C" int tuch_point_cloud_canary_hits(void* workspace, int* hits_host, int reset)
{
    TUCH_REQUIRE(workspace && hits_host, "tuch_point_cloud_canary_hits: null pointer");
    int32_t zero = 0;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(hits_host, workspace, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        (reset && hipMemcpy(workspace, &zero, sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)) {
        tuch_set_error("tuch_point_cloud_canary_hits: %s", hipGetErrorString(hipGetLastError()));
        return TUCH_ERR_HIP;
    }
    return TUCH_OK;
}
