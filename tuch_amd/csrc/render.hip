// Mesh renderer on the compute units: face ids, depth and shaded views of a batch of bodies, and the reference's contact
// colouring.
//
// Replaces what tuch/utils/renderer.py asks of pyrender / OpenGL (Renderer.__call__, renderer.py:174-271): an Instinct
// accelerator has no graphics pipeline.  Geometry, visibility and the vertex colours are reproduced; pyrender's
// physically based look is not (one ambient + one headlight term instead, see render_shade_kernel).
//
// Camera: utils/geometry.perspective_projection.  p = R_view v + t lands at (f p.x / p.z + cx, f p.y / p.z + cy); the
// pixel in row r, column c has its centre at (c + 0.5, r + 0.5).
//
// Four launches and one memset per call, whatever B and the number of views:
//   1. render_vertex_kernel, one thread per (body, vertex): the area-weighted vertex normal in the body frame, gathered
//      through the vertex -> faces lists in list order (no atomics), and for every view the projected position -- snapped
//      to 1/256 px as two integers for the coverage test, and as it is (float32 pixels) for the interpolation -- plus the
//      camera-space z.  Both later passes read THESE numbers, so that the shading pass recomputes the barycentrics the
//      coverage pass used.
//   2. render_raster_kernel, one lane per (body, view, triangle).  Coverage is exact: 64-bit integer edge functions of the
//      snapped corners at the pixel centres, the triangle oriented to positive area first (no back-face culling), and a
//      centre ON an edge counted in when the centre moved by (+eps, +eps^2) would be strictly inside -- the top-left rule:
//      a centre on a shared edge or vertex belongs to exactly one of the triangles around it, whatever their order or
//      winding.  A small bounding box (<= kLaneBox pixels: SMPL faces at 224^2 cover one to four) is walked by its lane; a
//      large one is handed to the whole wavefront, lanes over pixels, one such triangle after the other, so that a
//      full-frame triangle does not serialise in one lane.
//      Visibility is one 64-bit key per pixel, (float bits of z) << 32 | face id, merged with atomicMin: positive floats
//      order like their bits, so the nearest surface wins and the smaller face id at equal depth; the minimum is
//      associative and commutative: the result does not depend on the order of arrival.  A key that is already smaller is
//      not touched (plain read first; keys only ever decrease, a stale read can only cause a redundant atomic).
//      z is interpolated perspective-correctly: 1/z is linear in screen space.  The weights of the interpolation come
//      from the UNSNAPPED projections (clamped to the triangle: a centre inside the snapped triangle may lie up to
//      1/360 px outside the true one): on a face seen at a grazing angle the 1/512 px of the snapping would move depth by
//      3e-4 relative and the shading by more than one 8-bit level (measured).
//   3. render_shade_kernel, one thread per output pixel: face and z from the key, barycentrics again from the snapped
//      corners, perspective-correct interpolation of the vertex normals and colours,
//      rgb = albedo / 255 * min(1, 0.3 + 0.7 max(0, -n_z)), over the background or over white.
//
// The contact colours (renderer.py:199-224) for a batch: colors_bounds_kernel (per-axis minimum and maximum of a body, one
// workgroup each), colors_mark_*_kernel (the LAST pair that writes a vertex: atomicMax of the pair index, order-free) and
// colors_resolve_kernel (one thread per vertex).
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr float kNear = 1e-3f;            // metres: a triangle with a corner at or behind this plane is dropped whole
constexpr int kSubpixelBits = 8;          // 1/256 px
constexpr int kSub = 1 << kSubpixelBits;
constexpr int kHalf = kSub / 2;
constexpr float kMaxCoord = 536870912.0f; // 2^29 subpixels (2^21 px): beyond it a projection counts as not finite, which
                                          // keeps every edge function below 2^62
constexpr int kLaneBox = 32;              // bounding boxes of up to this many pixels are walked by one lane
constexpr int kMaxViews = 32;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kDefaultAlbedo = 230;       // renderer.py:185

struct Snapped { int x, y; float z; int ok; float fx, fy; };

// ------------------------------------------------------------------------------------------------ vertex pass
__global__ __launch_bounds__(kBlock) void render_vertex_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_off,
    const int32_t* __restrict__ vf_ids, int B, int V, int F, const float* __restrict__ cam_t,
    const float* __restrict__ view_rot, int n_views, float focal, float cx, float cy,
    int4* __restrict__ proj,               // [B,n_views,V]
    float2* __restrict__ projf,            // [B,n_views,V]
    float4* __restrict__ normals)          // [B,V]
{
    const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (size_t)B * V) return;
    const int b = (int)(k / V), v = (int)(k - (size_t)b * V);
    const float* vb = verts + (size_t)b * V * 3;
    const float x = vb[3 * v], y = vb[3 * v + 1], z = vb[3 * v + 2];

    // area-weighted normal: the sum of the cross products of the faces around the vertex, in list order
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    const int beg = vf_off[v], end = vf_off[v + 1];
    for (int e = beg; e < end; ++e) {
        const int f = vf_ids[e];
        if ((unsigned)f >= (unsigned)F) continue;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
        const float ax = vb[3 * i0], ay = vb[3 * i0 + 1], az = vb[3 * i0 + 2];
        const float ux = vb[3 * i1] - ax, uy = vb[3 * i1 + 1] - ay, uz = vb[3 * i1 + 2] - az;
        const float wx = vb[3 * i2] - ax, wy = vb[3 * i2 + 1] - ay, wz = vb[3 * i2 + 2] - az;
        const float gx = uy * wz - uz * wy, gy = uz * wx - ux * wz, gz = ux * wy - uy * wx;
        if (!(__builtin_isfinite(gx) && __builtin_isfinite(gy) && __builtin_isfinite(gz))) continue;   // a broken neighbour
        nx += gx; ny += gy; nz += gz;
    }
    const float len = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
    const float inv = len > 0.0f ? 1.0f / len : 0.0f;
    normals[k] = make_float4(nx * inv, ny * inv, nz * inv, 0.0f);

    const float tx = cam_t[3 * b], ty = cam_t[3 * b + 1], tz = cam_t[3 * b + 2];
    for (int w = 0; w < n_views; ++w) {
        const float* R = view_rot + 9 * w;
        const float px = R[0] * x + R[1] * y + R[2] * z + tx;
        const float py = R[3] * x + R[4] * y + R[5] * z + ty;
        const float pz = R[6] * x + R[7] * y + R[8] * z + tz;
        const float ux = focal * px / pz + cx, uy = focal * py / pz + cy;
        const float sx = ux * (float)kSub, sy = uy * (float)kSub;
        // (NaN fails every comparison)
        const bool ok = pz > kNear && pz < __builtin_inff() && __builtin_fabsf(sx) <= kMaxCoord &&
                        __builtin_fabsf(sy) <= kMaxCoord;
        int4 o;
        o.x = ok ? (int)__builtin_rintf(sx) : 0;
        o.y = ok ? (int)__builtin_rintf(sy) : 0;
        o.z = __float_as_int(ok ? pz : 0.0f);
        o.w = ok;
        proj[((size_t)b * n_views + w) * V + v] = o;
        projf[((size_t)b * n_views + w) * V + v] = make_float2(ok ? ux : 0.0f, ok ? uy : 0.0f);
    }
}

// ------------------------------------------------------------------------------------------------ coverage
// A triangle set up for the pixel tests: the three edge functions E_k(p) = A_k p.x + B_k p.y + C_k in subpixel units,
// oriented so that the interior is positive; E_0 belongs to the edge opposite corner 0, so E_k / area is the weight of
// corner k.
struct Setup {
    long long A[3], B[3], C[3];
    float inv_area;
    float iz[3];                   // 1 / z of the corners
    float fx[3], fy[3];            // the unsnapped projections, pixels
    int c0, c1, r0, r1;            // pixel columns / rows of the clipped bounding box, inclusive (c0 > c1: nothing)
};

__device__ __forceinline__ Snapped load_snapped(const int4* p, const float2* pf)
{
    const int4 q = *p;
    const float2 u = *pf;
    return Snapped{q.x, q.y, __int_as_float(q.z), q.w, u.x, u.y};
}

__device__ __forceinline__ bool setup_triangle(const Snapped& a, const Snapped& b, const Snapped& c, int H, int W, Setup& s)
{
    s.c0 = 0; s.c1 = -1; s.r0 = 0; s.r1 = -1;
    if (!(a.ok && b.ok && c.ok)) return false;
    const long long x[3] = {a.x, b.x, c.x}, y[3] = {a.y, b.y, c.y};
    long long area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
    if (area == 0) return false;
    const long long sgn = area > 0 ? 1 : -1;
    area *= sgn;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // the edge from corner k+1 to corner k+2: E(p) = (x2 - x1) (p.y - y1) - (y2 - y1) (p.x - x1)
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const long long dx = x[j] - x[i], dy = y[j] - y[i];
        s.A[k] = -sgn * dy;
        s.B[k] = sgn * dx;
        s.C[k] = sgn * (dy * x[i] - dx * y[i]);
    }
    s.inv_area = 1.0f / (float)area;
    s.iz[0] = 1.0f / a.z; s.iz[1] = 1.0f / b.z; s.iz[2] = 1.0f / c.z;
    s.fx[0] = a.fx; s.fx[1] = b.fx; s.fx[2] = c.fx;
    s.fy[0] = a.fy; s.fy[1] = b.fy; s.fy[2] = c.fy;
    const int xmin = min(a.x, min(b.x, c.x)), xmax = max(a.x, max(b.x, c.x));
    const int ymin = min(a.y, min(b.y, c.y)), ymax = max(a.y, max(b.y, c.y));
    // centres c * 256 + 128 inside [min, max]: arithmetic shifts are floor divisions
    s.c0 = max(0, (xmin - kHalf + kSub - 1) >> kSubpixelBits);
    s.c1 = min(W - 1, (xmax - kHalf) >> kSubpixelBits);
    s.r0 = max(0, (ymin - kHalf + kSub - 1) >> kSubpixelBits);
    s.r1 = min(H - 1, (ymax - kHalf) >> kSubpixelBits);
    return s.c0 <= s.c1 && s.r0 <= s.r1;
}

// Is the centre of pixel (row r, column c) covered?  e[k]: the edge functions there.
__device__ __forceinline__ bool covers(const Setup& s, int r, int c, long long e[3])
{
    const long long px = (long long)c * kSub + kHalf, py = (long long)r * kSub + kHalf;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e[k] = s.A[k] * px + s.B[k] * py + s.C[k];
        // on the edge: inside when a step to the right enters the triangle (A > 0), or along a horizontal edge a step down
        in = in && (e[k] > 0 || (e[k] == 0 && (s.A[k] > 0 || (s.A[k] == 0 && s.B[k] > 0))));
    }
    return in;
}

// Screen-space weights of the three corners at the centre of pixel (r, c), which the snapped triangle covers (e[k]: its
// edge functions there): the barycentrics of the UNSNAPPED triangle -- cross products of the corners relative to the
// centre --, clamped to [0,1] and renormalised (the nearest point of the triangle when the centre lies just outside it).
// A triangle whose unsnapped area vanishes falls back to the snapped weights e[k] / area.  Every operation is spelled out
// (no contraction left to the compiler): the two walks of the coverage pass and the shading pass must give the same bits.
#pragma clang fp contract(off)
__device__ __forceinline__ void weights_at(const Setup& s, int r, int c, const long long e[3], float w[3])
{
    const float qx = (float)c + 0.5f, qy = (float)r + 0.5f;
    const float ax = s.fx[0] - qx, ay = s.fy[0] - qy, bx = s.fx[1] - qx, by = s.fy[1] - qy, cx = s.fx[2] - qx, cy = s.fy[2] - qy;
    const float g0 = __builtin_fmaf(bx, cy, -(by * cx)), g1 = __builtin_fmaf(cx, ay, -(cy * ax)),
                g2 = __builtin_fmaf(ax, by, -(ay * bx));
    const float inv = 1.0f / ((g0 + g1) + g2);
    float w0 = fminf(fmaxf(g0 * inv, 0.0f), 1.0f), w1 = fminf(fmaxf(g1 * inv, 0.0f), 1.0f), w2 = fminf(fmaxf(g2 * inv, 0.0f), 1.0f);
    const float sum = (w0 + w1) + w2;
    if (sum >= 0.25f && sum <= 3.0f) {                       // (false for a NaN: 0 / 0 or inf * 0 above)
        const float n = 1.0f / sum;
        w[0] = w0 * n; w[1] = w1 * n; w[2] = w2 * n;
    } else {
        w[0] = (float)e[0] * s.inv_area; w[1] = (float)e[1] * s.inv_area; w[2] = (float)e[2] * s.inv_area;
    }
}

__device__ __forceinline__ float depth_at(const Setup& s, const float w[3])
{
    return 1.0f / __builtin_fmaf(w[2], s.iz[2], __builtin_fmaf(w[1], s.iz[1], w[0] * s.iz[0]));
}
#pragma clang fp contract(fast)

__device__ __forceinline__ void visit(const Setup& s, int r, int c, int W, unsigned long long* keys, int face)
{
    long long e[3];
    if (!covers(s, r, c, e)) return;
    float w[3];
    weights_at(s, r, c, e, w);
    const float z = depth_at(s, w);
    if (!(z > 0.0f && z < __builtin_inff())) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned int)face;
    unsigned long long* p = keys + (size_t)r * W + c;
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(p, key);
}

__device__ __forceinline__ long long shfl_ll(long long v, int lane)
{
    const int lo = __shfl((int)(unsigned int)(unsigned long long)v, lane);
    const int hi = __shfl((int)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo);
}

__global__ __launch_bounds__(kBlock) void render_raster_kernel(
    const int32_t* __restrict__ faces, const int4* __restrict__ proj, const float2* __restrict__ projf,
    int n_images /* B * n_views */, int V, int F, int H, int W, unsigned long long* keys /* [n_images,H,W] */)
{
    const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = k < (size_t)n_images * F;
    const int img = live ? (int)(k / F) : 0, f = live ? (int)(k - (size_t)img * F) : 0;
    Setup s;
    s.c0 = 0; s.c1 = -1; s.r0 = 0; s.r1 = -1;
    bool draw = false;
    if (live) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            const int4* pv = proj + (size_t)img * V;
            const float2* pf = projf + (size_t)img * V;
            draw = setup_triangle(load_snapped(pv + i0, pf + i0), load_snapped(pv + i1, pf + i1), load_snapped(pv + i2, pf + i2),
                                  H, W, s);
        }
    }
    const int bw = s.c1 - s.c0 + 1, bh = s.r1 - s.r0 + 1;
    const bool big = draw && (long long)bw * bh > kLaneBox;
    if (draw && !big) {
        unsigned long long* kimg = keys + (size_t)img * H * W;
        for (int r = s.r0; r <= s.r1; ++r)
            for (int c = s.c0; c <= s.c1; ++c) visit(s, r, c, W, kimg, f);
    }
    // the large boxes of this wavefront, one after the other, lanes over pixels
    unsigned long long todo = __builtin_amdgcn_ballot_w64(big);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        Setup t;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            t.A[e] = shfl_ll(s.A[e], src); t.B[e] = shfl_ll(s.B[e], src); t.C[e] = shfl_ll(s.C[e], src);
            t.iz[e] = __shfl(s.iz[e], src); t.fx[e] = __shfl(s.fx[e], src); t.fy[e] = __shfl(s.fy[e], src);
        }
        t.inv_area = __shfl(s.inv_area, src);
        t.c0 = __shfl(s.c0, src); t.c1 = __shfl(s.c1, src); t.r0 = __shfl(s.r0, src); t.r1 = __shfl(s.r1, src);
        const int timg = __shfl(img, src), tf = __shfl(f, src);
        const int tw = t.c1 - t.c0 + 1;
        const int n = tw * (t.r1 - t.r0 + 1);                 // <= 2^28 (render_sizes_ok)
        unsigned long long* kimg = keys + (size_t)timg * H * W;
        for (int q = lane; q < n; q += 64) {
            const int r = t.r0 + q / tw, c = t.c0 + q % tw;
            visit(t, r, c, W, kimg, tf);
        }
    }
}

// ------------------------------------------------------------------------------------------------ shading
__global__ __launch_bounds__(kBlock) void render_shade_kernel(
    const unsigned long long* __restrict__ keys, const int32_t* __restrict__ faces, const int4* __restrict__ proj,
    const float2* __restrict__ projf, const float4* __restrict__ normals, const float* __restrict__ view_rot, const uint8_t* __restrict__ colors,
    const float* __restrict__ background, unsigned int background_views, int B, int n_views, int V, int F, int H, int W,
    int32_t* __restrict__ out_face, float* __restrict__ out_depth, float* __restrict__ out_image)
{
    const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t hw = (size_t)H * W;
    if (k >= (size_t)B * n_views * hw) return;
    const int img = (int)(k / hw);
    const size_t pix = k - (size_t)img * hw;
    const int r = (int)(pix / W), c = (int)(pix - (size_t)r * W);
    const int b = img / n_views, w = img - b * n_views;
    const unsigned long long key = keys[k];
    float red, green, blue;
    if (key == kEmptyKey) {
        out_face[k] = -1;
        out_depth[k] = 0.0f;
        if (background && ((background_views >> w) & 1u)) {
            const float* bg = background + ((size_t)b * hw + pix) * 3;
            red = bg[0]; green = bg[1]; blue = bg[2];
        } else {
            red = green = blue = 1.0f;
        }
    } else {
        const int f = (int)(unsigned int)key;                  // written by the coverage pass: in range, corners valid
        const float z = __uint_as_float((unsigned int)(key >> 32));
        out_face[k] = f;
        out_depth[k] = z;
        const int id[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        const int4* pv = proj + (size_t)img * V;
        const float2* pf = projf + (size_t)img * V;
        Setup s;
        setup_triangle(load_snapped(pv + id[0], pf + id[0]), load_snapped(pv + id[1], pf + id[1]),
                       load_snapped(pv + id[2], pf + id[2]), H, W, s);
        long long e[3];
        covers(s, r, c, e);
        float ws[3];
        weights_at(s, r, c, e, ws);
        // perspective-correct weights: (w_k / z_k) z
        float wt[3], n[3] = {0.0f, 0.0f, 0.0f}, alb[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            wt[q] = ws[q] * s.iz[q] * z;
            const float4 nv = normals[(size_t)b * V + id[q]];
            n[0] += wt[q] * nv.x; n[1] += wt[q] * nv.y; n[2] += wt[q] * nv.z;
            if (colors) {
                const uint8_t* cv = colors + ((size_t)b * V + id[q]) * 3;
                alb[0] += wt[q] * (float)cv[0]; alb[1] += wt[q] * (float)cv[1]; alb[2] += wt[q] * (float)cv[2];
            }
        }
        if (!colors) alb[0] = alb[1] = alb[2] = (float)kDefaultAlbedo;
        const float* R = view_rot + 9 * w;
        const float len = __builtin_sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        const float nz = len > 0.0f ? (R[6] * n[0] + R[7] * n[1] + R[8] * n[2]) / len : 0.0f;
        // ambient 0.3 (renderer.py:229) + lights along the viewing direction (+z of this camera frame)
        const float shade = fminf(1.0f, 0.3f + 0.7f * fmaxf(0.0f, -nz));
        red = fminf(1.0f, alb[0] * (1.0f / 255.0f) * shade);
        green = fminf(1.0f, alb[1] * (1.0f / 255.0f) * shade);
        blue = fminf(1.0f, alb[2] * (1.0f / 255.0f) * shade);
    }
    out_image[3 * k] = red; out_image[3 * k + 1] = green; out_image[3 * k + 2] = blue;
}

// ------------------------------------------------------------------------------------------------ contact colours
// bounds [B,6]: per-axis minimum, then max_axis(v - min_axis) -- the float32 difference of the extremes, which IS the
// maximum of the float32 differences (rounding is monotonic).  Also presets the body's `last` entries to -1.
__global__ __launch_bounds__(kBlock) void colors_bounds_kernel(const float* __restrict__ verts, int V,
                                                              float* __restrict__ bounds, int32_t* __restrict__ last,
                                                              int n_last /* per body */)
{
    __shared__ float red[6][kBlock / 64];
    const int b = blockIdx.x;
    const float* vb = verts + (size_t)b * V * 3;
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int v = threadIdx.x; v < V; v += kBlock) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = vb[3 * v + a];
            if (x == x) { lo[a] = fminf(lo[a], x); hi[a] = fmaxf(hi[a], x); }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min_uniform(lo[a]), h = wave_max_uniform(hi[a]);
        if ((threadIdx.x & 63) == 0) { red[a][threadIdx.x >> 6] = l; red[3 + a][threadIdx.x >> 6] = h; }
    }
    for (int k = threadIdx.x; k < n_last; k += kBlock) last[(size_t)b * n_last + k] = -1;
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        float l = red[a][0], h = red[3 + a][0];
        for (int w = 1; w < kBlock / 64; ++w) { l = fminf(l, red[a][w]); h = fmaxf(h, red[3 + a][w]); }
        bounds[6 * b + a] = l;
        bounds[6 * b + 3 + a] = h - l;
    }
}

// pair form: the last pair of the body's list that names a vertex
__global__ __launch_bounds__(kBlock) void colors_mark_pairs_kernel(const int32_t* __restrict__ pair_off, const int32_t* __restrict__ c1,
                                                                  const int32_t* __restrict__ c2, int B, int V, int n_pairs,
                                                                  int32_t* last /* [B,V] */)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_pairs) return;
    int lo = 0, hi = B;                                      // the body b with pair_off[b] <= k < pair_off[b + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= k) lo = mid; else hi = mid;
    }
    const int b = lo, begin = pair_off[b];
    if (k < begin || k >= pair_off[b + 1]) return;           // offsets that do not ascend: nothing is written
    const int a = c1[k], c = c2[k];
    if ((unsigned)a >= (unsigned)V || (unsigned)c >= (unsigned)V) return;
    atomicMax(last + (size_t)b * V + a, k - begin);
    atomicMax(last + (size_t)b * V + c, k - begin);
}

// region form: the last active pair that names a region
__global__ __launch_bounds__(kBlock) void colors_mark_regions_kernel(const uint8_t* __restrict__ contact, const int32_t* __restrict__ pairs,
                                                                    const int32_t* __restrict__ region_first, int B, int P, int R, int V,
                                                                    int32_t* last /* [B,R] */)
{
    const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (size_t)B * P) return;
    const int b = (int)(k / P), p = (int)(k - (size_t)b * P);
    if (contact[k] != 1) return;
    const int r1 = pairs[2 * p], r2 = pairs[2 * p + 1];
    if ((unsigned)r1 >= (unsigned)R || (unsigned)r2 >= (unsigned)R) return;
    if ((unsigned)region_first[r1] >= (unsigned)V) return;   // an empty first region has no colour to give
    atomicMax(last + (size_t)b * R + r1, p);
    atomicMax(last + (size_t)b * R + r2, p);
}

__device__ __forceinline__ int meshcol(const float* vb, const float* bounds, int v, int a)
{
    // float32, in the reference's order: (v - min) * 255 / max, truncated
    const float d = vb[3 * v + a] - bounds[a];
    const float q = d * 255.0f / bounds[3 + a];
    return q >= 0.0f ? (int)fminf(q, 255.0f) : 0;            // (0 / 0 on a flat axis: 0)
}

__global__ __launch_bounds__(kBlock) void colors_resolve_kernel(
    const float* __restrict__ verts, const float* __restrict__ bounds, const int32_t* __restrict__ last, int B, int V,
    const int32_t* __restrict__ pair_off, const int32_t* __restrict__ c1, const int32_t* __restrict__ c2,        // pair form
    const int32_t* __restrict__ pairs, const int32_t* __restrict__ region_first, const int32_t* __restrict__ vreg_off,
    const int32_t* __restrict__ vreg, int R,                                                                         // region form
    uint8_t* __restrict__ colors)
{
    const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (size_t)B * V) return;
    const int b = (int)(k / V), v = (int)(k - (size_t)b * V);
    const float* vb = verts + (size_t)b * V * 3;
    const float* bd = bounds + 6 * b;
    int rgb[3] = {kDefaultAlbedo, kDefaultAlbedo, kDefaultAlbedo};
    if (pair_off) {
        const int w = last[k];
        if (w >= 0) {
            const int a = c1[pair_off[b] + w], c = c2[pair_off[b] + w];
#pragma unroll
            for (int x = 0; x < 3; ++x) rgb[x] = (meshcol(vb, bd, a, x) + meshcol(vb, bd, c, x)) >> 1;
        }
    } else {
        int w = -1;
        for (int e = vreg_off[v]; e < vreg_off[v + 1]; ++e) {
            const int r = vreg[e];
            if ((unsigned)r < (unsigned)R) w = max(w, last[(size_t)b * R + r]);
        }
        if (w >= 0) {
            const int src = region_first[pairs[2 * w]];
#pragma unroll
            for (int x = 0; x < 3; ++x) rgb[x] = meshcol(vb, bd, src, x);
        }
    }
    colors[3 * k] = (uint8_t)rgb[0]; colors[3 * k + 1] = (uint8_t)rgb[1]; colors[3 * k + 2] = (uint8_t)rgb[2];
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct RenderLayout { size_t keys, proj, projf, normals, total; };
RenderLayout render_layout(int B, int n_views, int V, int H, int W)
{
    RenderLayout l;
    l.keys = 0;
    l.proj = align256((size_t)B * n_views * H * W * sizeof(unsigned long long));
    l.projf = l.proj + align256((size_t)B * n_views * V * sizeof(int4));
    l.normals = l.projf + align256((size_t)B * n_views * V * sizeof(float2));
    l.total = l.normals + align256((size_t)B * V * sizeof(float4));
    return l;
}

bool render_sizes_ok(int B, int n_views, int V, int F, int H, int W)
{
    return B >= 0 && n_views >= 1 && n_views <= kMaxViews && V >= 1 && F >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 &&
           (double)B * n_views * H * W < 2147483648.0 && (double)B * n_views * F < 2147483648.0 * kBlock &&
           (double)B * n_views * V < 2147483648.0;
}

}  // namespace

extern "C" size_t tuch_render_workspace_bytes(int B, int n_views, int V, int F, int H, int W)
{
    if (!render_sizes_ok(B, n_views, V, F, H, W)) return 0;
    return render_layout(B, n_views, V, H, W).total;
}

extern "C" int tuch_render_mesh(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_ids, int B,
                                int V, int F, const float* cam_t, const float* view_rot, int n_views, float focal, float cx,
                                float cy, int H, int W, const uint8_t* colors, const float* background,
                                unsigned int background_views, int32_t* face, float* depth, float* image, void* workspace,
                                size_t workspace_bytes, void* stream)
{
    TUCH_REQUIRE(render_sizes_ok(B, n_views, V, F, H, W),
                 "tuch_render_mesh: bad sizes B %d, views %d (1 to %d), V %d, F %d, image %d x %d", B, n_views, kMaxViews, V, F,
                 H, W);
    if (B == 0) return TUCH_OK;
    TUCH_REQUIRE(verts && faces && vf_off && vf_ids && cam_t && view_rot && face && depth && image && workspace,
                 "tuch_render_mesh: null pointer");
    TUCH_REQUIRE(focal == focal && cx == cx && cy == cy, "tuch_render_mesh: the camera is not a number");
    const RenderLayout l = render_layout(B, n_views, V, H, W);
    if (workspace_bytes < l.total) {
        tuch_set_error("tuch_render_mesh: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
        return TUCH_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + l.keys);
    int4* proj = (int4*)((char*)workspace + l.proj);
    float2* projf = (float2*)((char*)workspace + l.projf);
    float4* normals = (float4*)((char*)workspace + l.normals);
    const size_t n_pix = (size_t)B * n_views * H * W;
    if (hipMemsetAsync(keys, 0xff, n_pix * sizeof(unsigned long long), s) != hipSuccess) {
        tuch_set_error("tuch_render_mesh: hipMemsetAsync failed");
        return TUCH_ERR_HIP;
    }
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)(((size_t)B * V + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, verts,
                       faces, vf_off, vf_ids, B, V, F, cam_t, view_rot, n_views, focal, cx, cy, proj, projf, normals);
    hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)(((size_t)B * n_views * F + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       s, faces, proj, projf, B * n_views, V, F, H, W, keys);
    hipLaunchKernelGGL(render_shade_kernel, dim3((unsigned)((n_pix + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, keys, faces,
                       proj, projf, normals, view_rot, colors, background, background_views, B, n_views, V, F, H, W, face, depth,
                       image);
    return tuch_check_launch("tuch_render_mesh");
}

extern "C" size_t tuch_contact_vertex_colors_workspace_bytes(int B, int V, int R)
{
    if (B < 0 || V < 1 || R < 0) return 0;
    return align256((size_t)B * 6 * sizeof(float)) + align256((size_t)B * (size_t)(V > R ? V : R) * sizeof(int32_t));
}

extern "C" int tuch_contact_vertex_colors(const float* verts, int B, int V, const int32_t* pair_off, const int32_t* c1,
                                          const int32_t* c2, int n_pairs, const uint8_t* contact, const int32_t* pairs, int P,
                                          const int32_t* region_first, const int32_t* vreg_off, const int32_t* vreg, int R,
                                          uint8_t* colors, void* workspace, size_t workspace_bytes, void* stream)
{
    TUCH_REQUIRE(B >= 0 && V >= 1 && (double)B * V < 2147483648.0, "tuch_contact_vertex_colors: bad sizes B %d, V %d", B, V);
    if (B == 0) return TUCH_OK;
    TUCH_REQUIRE(verts && colors && workspace, "tuch_contact_vertex_colors: null pointer");
    const bool pair_form = pair_off != nullptr;
    TUCH_REQUIRE(pair_form != (contact != nullptr), "tuch_contact_vertex_colors: give the pair lists or the region form, not both");
    if (pair_form) {
        TUCH_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || (c1 && c2)), "tuch_contact_vertex_colors: %d pairs without lists", n_pairs);
    } else {
        TUCH_REQUIRE(pairs && region_first && vreg_off && vreg && P >= 1 && R >= 1 && (double)B * P < 2147483648.0,
                     "tuch_contact_vertex_colors: the region form needs pairs, region_first and the vertex -> regions table");
    }
    const size_t need = tuch_contact_vertex_colors_workspace_bytes(B, V, pair_form ? 0 : R);
    if (workspace_bytes < need) {
        tuch_set_error("tuch_contact_vertex_colors: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return TUCH_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float* bounds = (float*)workspace;
    int32_t* last = (int32_t*)((char*)workspace + align256((size_t)B * 6 * sizeof(float)));
    const int n_last = pair_form ? V : R;
    hipLaunchKernelGGL(colors_bounds_kernel, dim3(B), dim3(kBlock), 0, s, verts, V, bounds, last, n_last);
    if (pair_form) {
        if (n_pairs > 0)
            hipLaunchKernelGGL(colors_mark_pairs_kernel, dim3(ceil_div(n_pairs, kBlock)), dim3(kBlock), 0, s, pair_off, c1, c2, B,
                               V, n_pairs, last);
    } else {
        hipLaunchKernelGGL(colors_mark_regions_kernel, dim3((unsigned)(((size_t)B * P + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           contact, pairs, region_first, B, P, R, V, last);
    }
    hipLaunchKernelGGL(colors_resolve_kernel, dim3((unsigned)(((size_t)B * V + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, verts,
                       bounds, last, B, V, pair_form ? pair_off : nullptr, c1, c2, pairs, region_first, vreg_off, vreg, R, colors);
    return tuch_check_launch("tuch_contact_vertex_colors");
}
