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
//   pc_clear_kernel    the cell and block tables of every body <- 0 (a kernel, not a memset: a captured loop then holds
//                      kernel nodes only)
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
// The query (pc_search): one query per lane, 64 consecutive queries of one body per wavefront.  A lane walks the blocks in
// Chebyshev rings around the block of its own (clamped) cell; a block is opened when it holds points and its bound admits
// it, then each of its cells likewise, then pc_d2 on the cell's points.  The walk ends after ring r when the ring bound
// (below) exceeds the lane's key, or when the grid is exhausted.
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
// is skipped by the same test on one or two axes' shares alone (a sum of fewer non-negative terms, rounded: not larger).  A query outside the grid needs
// nothing special (t_q is not clamped for the bound); one whose t_q overflows has slack +inf, l = 0 and prunes nothing.
//
// The hint.  hint[b,n] in [0, Q) that names a valid point (checked on the caller's arrays before anything else is
// addressed) whose d2 is finite and within tau enters as an ordinary key -- the exact d2 to that point, which the full
// sweep computes too, so it cannot undercut the sweep's minimum; it only shortens the walk.  Anything else takes the
// unhinted path.  hint may alias the index output: a lane reads its own entry before it writes it.
//
// The term (pc_fit_kernel; tuch_point_cloud_fit_terms): the query for q = verts[b,v] + transl[b], then per vertex
// g_v = scale w_v rho'(d2_v) / sum w and grad_verts[b,v] = 2 g_v (q - s) written by the lane that owns the row (no
// atomics); the per-body loss, the normaliser and grad_transl = sum_v grad_verts[b,v] cross to the workgroup that arrives
// last (mesh_fit.hip's ticket scheme, here with a release fence / acquire fence pair) and are added in chunk order, the
// total in a fixed tree: no float atomics, the same bits in either mode of tuch_set_deterministic and for a body alone or
// in a batch.  A vertex of weight 0 is not computed from; one without winner contributes rho(tau^2) when tau is given and
// the cloud is not empty, else 0, with a zero gradient row; a body with an empty cloud or without weight has loss 0.
#include "workspace.h"
#include <math.h>
#include <string.h>

#define TUCH_SCAN_RHO_SQUARED 0
#define TUCH_SCAN_RHO_DISTANCE 1
#define TUCH_SCAN_RHO_GMOF 2

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kCtl = 64;                 // control words in front of the headers: [0] guard words found changed
constexpr int kHead = 16;                // words per body header
constexpr int kPart = 8;                 // floats per partial: sum w rho, grad_transl.xyz, sum w, 3 unused
constexpr int kMaxRes = 256;
constexpr float kPcMargin = 9.5367431640625e-7f;       // M = 2^-20
constexpr float kPcMinCell = 1e-6f;
constexpr float kPcNormal = 1e-30f;
constexpr float kPcMaxD2 = 3.402823466e+38f;             // the largest finite d2: only a finite d2 can win
constexpr unsigned long long kPcNoKey = 0x7f800000ffffffffull;      // d2 = +inf, index = -1

enum { H_OX = 0, H_OY, H_OZ, H_CELL, H_INV, H_DX, H_DY, H_DZ, H_N, H_RES };

typedef __attribute__((address_space(1))) float gfloat;

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
    l.partial = tuch_ws_take(o, (size_t)B * ceil_div(N, kBlock) * kPart * sizeof(float));
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

__global__ __launch_bounds__(kBlock) void pc_clear_kernel(int32_t* __restrict__ tables, size_t n)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) tables[i] = 0;
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
    return lb > __uint_as_float((uint32_t)(best >> 32)) && lb >= kPcNormal;
}

// The smallest key of query (qx, qy, qz), finite, against the cloud of body b; `best` arrives as the starting key (no
// key: (limit bits, -1) with limit = tau^2 or FLT_MAX; or the hinted key).  A candidate needs d2 <= limit.
static __device__ unsigned long long pc_search(const PcTables& w, int b, int Q, float qx, float qy, float qz, float limit,
                                               unsigned long long best)
{
    const PcGrid g = pc_grid(w.head, b);
    const int n = pc_clampi(g.n, 0, Q);
    if (n == 0) return best;
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
        if (r > 1 && pc_out(pc_sq(g.cell, pc_gap(0.0f, 4 * (r - 1), 4 * (r - 1) + 1, slack)), best)) break;
        const int z0 = hz - r < 0 ? 0 : hz - r, z1 = hz + r > g.cdz - 1 ? g.cdz - 1 : hz + r;
        const int y0 = hy - r < 0 ? 0 : hy - r, y1 = hy + r > g.cdy - 1 ? g.cdy - 1 : hy + r;
        const int x0 = hx - r < 0 ? 0 : hx - r, x1 = hx + r > g.cdx - 1 ? g.cdx - 1 : hx + r;
        for (int bz = z0; bz <= z1; ++bz) {
            const float lz = pc_sq(g.cell, pc_gap(tz, 4 * bz, 4 * bz + 4, slack));
            if (pc_out(lz, best)) continue;                          // (one axis' share alone: the whole slab is out)
            const bool zface = bz - hz == r || hz - bz == r;
            for (int by = y0; by <= y1; ++by) {
                const float lyz = pc_add(pc_sq(g.cell, pc_gap(ty, 4 * by, 4 * by + 4, slack)), lz);
                if (pc_out(lyz, best)) continue;
                const bool face = zface || by - hy == r || hy - by == r;
                // the shell of the ring: whole rows on its faces, else the two end blocks
                const int step = face ? 1 : 2 * r;
                for (int bx = face ? x0 : (hx - r >= 0 ? hx - r : hx + r); bx <= x1; bx += step) {
                    if (pc_table(w, base + fine + ((long long)bz * g.cdy + by) * g.cdx + bx) <= 0) continue;
                    // (the sum's order differs from a cell's below; both are bounds of their own)
                    if (pc_out(pc_add(pc_sq(g.cell, pc_gap(tx, 4 * bx, 4 * bx + 4, slack)), lyz), best)) continue;
                    const int cz1 = 4 * bz + 4 < g.dz ? 4 * bz + 4 : g.dz, cy1 = 4 * by + 4 < g.dy ? 4 * by + 4 : g.dy,
                              cx1 = 4 * bx + 4 < g.dx ? 4 * bx + 4 : g.dx;
                    for (int cz = 4 * bz; cz < cz1; ++cz) {
                        const float mz = pc_sq(g.cell, pc_gap(tz, cz, cz + 1, slack));
                        if (pc_out(mz, best)) continue;
                        for (int cy = 4 * by; cy < cy1; ++cy) {
                            const float myz = pc_add(pc_sq(g.cell, pc_gap(ty, cy, cy + 1, slack)), mz);
                            if (pc_out(myz, best)) continue;
                            const long long row = base + ((long long)cz * g.dy + cy) * g.dx;
                            for (int cx = 4 * bx; cx < cx1; ++cx) {
                                const long long c = row + cx;
                                const int end = pc_clampi(pc_table(w, c), 0, n);
                                const int begin = c == base ? 0 : pc_clampi(pc_table(w, c - 1), 0, n);
                                if (begin >= end) continue;
                                if (pc_out(pc_add(pc_sq(g.cell, pc_gap(tx, cx, cx + 1, slack)), myz), best)) continue;
                                for (int p = begin; p < end; ++p) {
                                    const float4 s = pts[p];
                                    const float d2 = pc_d2(qx, qy, qz, s.x, s.y, s.z);
                                    const unsigned long long key =
                                        ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)__float_as_int(s.w);
                                    if (d2 <= limit && key < best) best = key;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    return best;
}

// The whole query of one lane: the starting key, the hint, the search.  Returns the key; (uint32_t)key == ~0u: no winner.
static __device__ __forceinline__ unsigned long long pc_query(const PcTables& w, const float* __restrict__ points,
                                                              const int32_t* __restrict__ counts,
                                                              const float* __restrict__ weights, int b, int Q, float qx,
                                                              float qy, float qz, int hint, float limit)
{
    unsigned long long best = ((unsigned long long)__float_as_uint(limit) << 32) | 0xffffffffull;
    if (!pc_finite3(qx, qy, qz)) return best;
    float sx, sy, sz;
    if (hint >= 0 && hint < Q && pc_valid(points, counts, weights, b, Q, hint, sx, sy, sz)) {
        const float d2 = pc_d2(qx, qy, qz, sx, sy, sz);
        if (d2 <= limit) best = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)hint;
    }
    return pc_search(w, b, Q, qx, qy, qz, limit, best);
}

__global__ __launch_bounds__(kBlock) void pc_nearest_kernel(PcTables w, const float* __restrict__ points,
                                                           const int32_t* __restrict__ counts,
                                                           const float* __restrict__ weights,
                                                           const float* __restrict__ queries, const float* __restrict__ shift,
                                                           const int32_t* __restrict__ query_counts, const int32_t* hint,
                                                           float limit, int Q, int N, float* __restrict__ d2_out,
                                                           int32_t* index_out)
{
    const int b = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const size_t o = (size_t)b * N + i;
    int count = N;
    if (query_counts) count = pc_clampi(query_counts[b], 0, N);
    unsigned long long best = kPcNoKey;
    if (i < count) {
        const int h = hint ? hint[o] : -1;
        float qx = queries[o * 3], qy = queries[o * 3 + 1], qz = queries[o * 3 + 2];
        if (shift) {
            qx = pc_add(qx, shift[3 * b]); qy = pc_add(qy, shift[3 * b + 1]); qz = pc_add(qz, shift[3 * b + 2]);
        }
        best = pc_query(w, points, counts, weights, b, Q, qx, qy, qz, h, limit);
    }
    const bool won = (uint32_t)best != 0xffffffffu;
    d2_out[o] = won ? __uint_as_float((uint32_t)(best >> 32)) : __builtin_inff();
    index_out[o] = won ? (int32_t)(uint32_t)best : -1;
}

// ---------------------------------------------------------------------------------------------------------- the term
#pragma clang fp contract(fast)

// Sum over the 64 lanes, valid in lane 0, in a fixed order.
static __device__ __forceinline__ float pc_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// rho(d2) and its derivative, as scan_fit.hip's ('distance' has derivative 0 at d2 = 0)
static __device__ __forceinline__ void pc_rho(int rho, float sigma2, float d2, float& value, float& slope)
{
    if (rho == TUCH_SCAN_RHO_SQUARED) {
        value = d2;
        slope = 1.0f;
    } else if (rho == TUCH_SCAN_RHO_DISTANCE) {
        value = __builtin_sqrtf(d2);
        slope = value > 0.0f ? 0.5f / value : 0.0f;
    } else {
        const float q = sigma2 / (sigma2 + d2);
        value = q * d2;
        slope = q * q;
    }
}

// vertex weights: layout 0 none (ones), 1 [V], 2 [B,V]
static __device__ __forceinline__ float pc_weight(const float* __restrict__ vw, int layout, int b, int V, int v)
{
    return layout == 0 ? 1.0f : vw[(layout == 2 ? (size_t)b * V : (size_t)0) + v];
}

__global__ __launch_bounds__(kBlock) void pc_fit_kernel(PcTables w, const float* __restrict__ points,
                                                       const int32_t* __restrict__ counts, const float* __restrict__ weights,
                                                       const float* __restrict__ verts, const float* __restrict__ transl,
                                                       const int32_t* hint, float limit, int has_tau, int B, int Q, int V,
                                                       const float* __restrict__ vw, int layout, int rho, float sigma2,
                                                       float scale, float* __restrict__ d2_out, int32_t* index_out,
                                                       float* partial, int* ticket, float* __restrict__ per_body,
                                                       float* __restrict__ total, float* __restrict__ grad_verts,
                                                       float* __restrict__ grad_transl)
{
    __shared__ float red[kWaves][4];
    __shared__ float s_wsum;
    __shared__ float tree[kBlock];
    __shared__ bool last;
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x, chunks = gridDim.x;
    // the normaliser: this body's vertex weights in one fixed order (the same bits in every workgroup of the body)
    float wsum = (float)V;
    if (layout != 0) {
        float acc = 0.0f;
        for (int i = t; i < V; i += kBlock) acc += pc_weight(vw, layout, b, V, i);
        acc = pc_wave_sum(acc);
        if ((t & 63) == 0) red[t >> 6][0] = acc;
        __syncthreads();
        if (t == 0) {
            float a = red[0][0];
#pragma unroll
            for (int j = 1; j < kWaves; ++j) a += red[j][0];
            s_wsum = a;
        }
        __syncthreads();
        wsum = s_wsum;
        __syncthreads();                                      // (red is written again below)
    }
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
            qx = pc_add(verts[o * 3], transl[3 * b]);
            qy = pc_add(verts[o * 3 + 1], transl[3 * b + 1]);
            qz = pc_add(verts[o * 3 + 2], transl[3 * b + 2]);
            best = pc_query(w, points, counts, weights, b, Q, qx, qy, qz, h, limit);
        }
        const bool won = (uint32_t)best != 0xffffffffu;
        const float d2 = won ? __uint_as_float((uint32_t)(best >> 32)) : __builtin_inff();
        const int idx = won ? (int32_t)(uint32_t)best : -1;
        d2_out[o] = d2;
        index_out[o] = idx;
        if (won) {
            float value, slope;
            pc_rho(rho, sigma2, d2, value, slope);
            s = wv * value;
            const float g2 = 2.0f * (scale * wv * slope / wsum);
            const float* p = points + ((size_t)b * Q + pc_clampi(idx, 0, Q - 1)) * 3;
            ex = g2 * (qx - p[0]); ey = g2 * (qy - p[1]); ez = g2 * (qz - p[2]);
        } else if (live && has_tau) {
            float value, slope;
            pc_rho(rho, sigma2, limit, value, slope);
            s = wv * value;
        }
        float* gv = grad_verts + o * 3;
        gv[0] = ex; gv[1] = ey; gv[2] = ez;
    }
    float sx = pc_wave_sum(ex), sy = pc_wave_sum(ey), sz = pc_wave_sum(ez);
    s = pc_wave_sum(s);
    if ((t & 63) == 0) {
        float* r = red[t >> 6];
        r[0] = s; r[1] = sx; r[2] = sy; r[3] = sz;
    }
    __syncthreads();
    if (t < 5) {
        float acc = wsum;
        if (t < 4) {
            acc = red[0][t];
#pragma unroll
            for (int j = 1; j < kWaves; ++j) acc += red[j][t];
        }
        __hip_atomic_store((gfloat*)partial + ((size_t)b * chunks + c) * kPart + t, acc, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");    // the partial is visible before the ticket is taken
    }
    __syncthreads();
    if (t == 0) {
        last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == chunks * B - 1;
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    float mine = 0.0f;
    for (int idx = t; idx < 4 * B; idx += kBlock) {           // (body, component); the stride keeps a thread on one component
        const int body = idx >> 2, k = idx & 3;
        const gfloat* p = (const gfloat*)partial + (size_t)body * chunks * kPart + k;
        float acc = 0.0f;
        for (int j = 0; j < chunks; ++j) acc += __hip_atomic_load(p + kPart * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            const float n = __hip_atomic_load((const gfloat*)partial + (size_t)body * chunks * kPart + 4, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
            const float value = n != 0.0f ? scale * (acc / n) : 0.0f;
            per_body[body] = value;
            mine += value;
        } else {
            grad_transl[3 * body + k - 1] = acc;
        }
    }
    tree[t] = mine;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (t < h) tree[t] += tree[t + h];
        __syncthreads();
    }
    if (t == 0) {
        total[0] = tree[0];
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
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

}  // namespace

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
    hipLaunchKernelGGL(pc_clear_kernel, dim3((unsigned)((ints + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tables, ints);
    hipLaunchKernelGGL(pc_header_kernel, dim3(B), dim3(kBlock), 0, s, points, counts, weights, Q, resolution, head);
    const dim3 grid(ceil_div(Q, kBlock), B);
    hipLaunchKernelGGL(pc_file_kernel<false>, grid, dim3(kBlock), 0, s, points, counts, weights, Q, resolution,
                       (const uint32_t*)head, tables, sorted);
    hipLaunchKernelGGL(pc_scan_kernel, dim3(B), dim3(kBlock), 0, s, (const uint32_t*)head, resolution, tables);
    hipLaunchKernelGGL(pc_file_kernel<true>, grid, dim3(kBlock), 0, s, points, counts, weights, Q, resolution,
                       (const uint32_t*)head, tables, sorted);
    return tuch_check_launch("tuch_point_cloud_build");
}

extern "C" int tuch_point_cloud_nearest(const void* workspace, size_t workspace_bytes, const float* points,
                                        const int32_t* counts, const float* weights, const float* queries,
                                        const float* shift, const int32_t* query_counts, const int32_t* hint,
                                        float max_distance, int B, int Q, int N, float* d2, int32_t* index, void* stream)
{
    TUCH_REQUIRE(workspace && points && queries && d2 && index, "tuch_point_cloud_nearest: null pointer");
    TUCH_REQUIRE(pc_sizes_ok(B, Q, N), "tuch_point_cloud_nearest: bad sizes B=%d Q=%d N=%d", B, Q, N);
    tuch_ws_scope scope(g_pc_canary != 0);
    const size_t need = pc_layout(B, Q, 1).total;
    if (workspace_bytes < need) {
        tuch_set_error("tuch_point_cloud_nearest: workspace %zu < %zu bytes", workspace_bytes, need);
        return TUCH_ERR_WORKSPACE;
    }
    const float limit = max_distance > 0.0f ? fminf(max_distance * max_distance, kPcMaxD2) : kPcMaxD2;
    hipLaunchKernelGGL(pc_nearest_kernel, dim3(ceil_div(N, kBlock), B), dim3(kBlock), 0, (hipStream_t)stream,
                       pc_tables((void*)workspace, workspace_bytes, B, Q), points, counts, weights, queries, shift,
                       query_counts, hint, limit, Q, N, d2, index);
    return tuch_check_launch("tuch_point_cloud_nearest");
}

extern "C" int tuch_point_cloud_fit_terms(const void* workspace, size_t workspace_bytes, const float* points,
                                          const int32_t* counts, const float* weights, const float* verts,
                                          const float* transl, const int32_t* hint, float max_distance, int B, int Q, int V,
                                          const float* vertex_weights, int vertex_weight_layout, int rho, float sigma,
                                          float scale, float* d2, int32_t* index, int* ticket, float* per_body, float* total,
                                          float* grad_verts, float* grad_transl, void* scratch, size_t scratch_bytes,
                                          void* stream)
{
    TUCH_REQUIRE(workspace && points && verts && transl && d2 && index && ticket && per_body && total && grad_verts &&
                     grad_transl && scratch,
                 "tuch_point_cloud_fit_terms: null pointer");
    TUCH_REQUIRE(pc_sizes_ok(B, Q, V), "tuch_point_cloud_fit_terms: bad sizes B=%d Q=%d V=%d", B, Q, V);
    TUCH_REQUIRE(vertex_weight_layout >= 0 && vertex_weight_layout <= 2 && (vertex_weight_layout == 0 || vertex_weights),
                 "tuch_point_cloud_fit_terms: vertex weight layout %d (0 none, 1 [V], 2 [B,V]) with weights %p",
                 vertex_weight_layout, (const void*)vertex_weights);
    TUCH_REQUIRE(rho == TUCH_SCAN_RHO_SQUARED || rho == TUCH_SCAN_RHO_DISTANCE || (rho == TUCH_SCAN_RHO_GMOF && sigma > 0.0f),
                 "tuch_point_cloud_fit_terms: rho %d (0 squared, 1 distance, 2 gmof with sigma > 0; sigma = %g)", rho,
                 (double)sigma);
    tuch_ws_scope scope(g_pc_canary != 0);
    const size_t need = pc_layout(B, Q, 1).total;
    const PcScratch sl = scope.record(0, [&] { return pc_scratch(B, V); });
    if (workspace_bytes < need || scratch_bytes < sl.total) {
        tuch_set_error("tuch_point_cloud_fit_terms: workspace %zu < %zu or scratch %zu < %zu bytes", workspace_bytes, need,
                       scratch_bytes, sl.total);
        return TUCH_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const PcTables w = pc_tables((void*)workspace, workspace_bytes, B, Q);
    scope.arm(scratch, (int32_t*)w.head, s);
    const float limit = max_distance > 0.0f ? fminf(max_distance * max_distance, kPcMaxD2) : kPcMaxD2;
    hipLaunchKernelGGL(pc_fit_kernel, dim3(ceil_div(V, kBlock), B), dim3(kBlock), 0, s, w, points, counts, weights, verts,
                       transl, hint, limit, max_distance > 0.0f ? 1 : 0, B, Q, V, vertex_weights, vertex_weight_layout, rho,
                       sigma * sigma, scale, d2, index, (float*)((char*)scratch + sl.partial), ticket, per_body, total,
                       grad_verts, grad_transl);
    return tuch_check_launch("tuch_point_cloud_fit_terms");
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
