// Fitting the body model to target meshes in correspondence (tuch/utils/smplxtosmpl_mtp.py:58,100-101):
//   tuch_vertex_fit_terms  the data term of one iteration, loss_b = sum_v w_v |verts_v + transl - target_v| / sum_v w_v,
//                          the total over the bodies and the unit gradients w.r.t. vertices and translation: ONE launch
//   tuch_mesh_transfer     out = M src for a sparse M in CSR form (the [6890 x 10475] SMPL-X -> SMPL matrix of :58)
#include "common.h"

namespace {

constexpr int kBlock = 256;              // four wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 1024;             // vertices per workgroup: V = 6890, B = 64 -> 7 x 64 = 448 workgroups
constexpr int kPer = kChunk / kBlock;    // vertices per thread

typedef __attribute__((address_space(1))) float gfloat;

// partial: [B][chunks][4] = (sum w |d|, sum g_x, sum g_y, sum g_z) of one workgroup.  They cross to the workgroup that
// arrives last as agent-scope (write-through) stores, drained before the ticket is taken, and agent-scope loads behind
// it; that workgroup leaves the ticket zero: it adds every body's chunks up in chunk order and the bodies in a fixed tree
// -- no float atomics, the four per-body sums and the total are the same bits on every call, in either mode of
// tuch_set_deterministic.  The hand-over is the drain form whose argument stands above fit_reduce_tail (fit_reduce.h),
// which the scan and the cloud term call.  This kernel keeps a tail of its own because the normaliser is a host
// argument here and a partial is 4 floats: with fit_reduce_tail's 8-float partials (the normaliser in slot 4) the term
// alone at batch 64, V = 6890 measured 13.5 us against 12.3 us, 0.85 us of it from the wider partials by themselves
// (the workgroup that arrives last reads them one dependent round trip per chunk).
template <bool kWeighted>
__global__ __launch_bounds__(kBlock) void vertex_fit_kernel(
    const float* __restrict__ verts, const float* __restrict__ transl, const float* __restrict__ target,
    const float* __restrict__ weights, int B, int V, float wsum, float* partial, int* ticket,
    float* __restrict__ loss, float* __restrict__ total, float* __restrict__ g_verts, float* __restrict__ g_transl)
{
    __shared__ float red[kWaves][4];
    __shared__ float tree[kBlock];
    __shared__ bool last;
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x, chunks = gridDim.x;
    const float tx = transl[3 * b], ty = transl[3 * b + 1], tz = transl[3 * b + 2];
    // the chunk's loads are issued before anything is computed from them (kPer independent vertices per thread: the kernel
    // is a few microseconds of memory latency, not of arithmetic); a vertex of weight 0 may be read -- its target may be
    // anything -- but nothing is computed from it
    float w[kPer], vx[kPer], vy[kPer], vz[kPer], qx[kPer], qy[kPer], qz[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {                      // (no branch between the loads: past the end the last vertex again)
        const int i = min(c * kChunk + k * kBlock + t, V - 1);
        const size_t at = ((size_t)b * V + i) * 3;
        w[k] = kWeighted ? weights[i] : 1.0f;
        vx[k] = verts[at]; vy[k] = verts[at + 1]; vz[k] = verts[at + 2];
        qx[k] = target[at]; qy[k] = target[at + 1]; qz[k] = target[at + 2];
    }
    float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = c * kChunk + k * kBlock + t;
        if (i >= V) break;
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (w[k] != 0.f) {
            const float dx = (vx[k] + tx) - qx[k], dy = (vy[k] + ty) - qy[k], dz = (vz[k] + tz) - qz[k];
            // (spelled out: left to the compiler, each unrolled copy may contract the sum its own way, and a vertex's
            // gradient row would depend on where in the chunk it sits)
            const float n = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
            s += w[k] * n;
            if (n > 0.f) {                                // torch.norm's subgradient at 0: a zero row
                const float f = w[k] / (n * wsum);
                ox = f * dx; oy = f * dy; oz = f * dz;
            }
        }
        float* g = g_verts + ((size_t)b * V + i) * 3;
        g[0] = ox; g[1] = oy; g[2] = oz;
        gx += ox; gy += oy; gz += oz;
    }
    s = wave_sum_lane0(s); gx = wave_sum_lane0(gx); gy = wave_sum_lane0(gy); gz = wave_sum_lane0(gz);
    if ((t & 63) == 0) {
        float* r = red[t >> 6];
        r[0] = s; r[1] = gx; r[2] = gy; r[3] = gz;
    }
    __syncthreads();
    if (t < 4) {
        float acc = red[0][t];
#pragma unroll
        for (int j = 1; j < kWaves; ++j) acc += red[j][t];
        __hip_atomic_store((gfloat*)partial + ((size_t)b * chunks + c) * 4 + t, acc, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    // (wave 0 holds the four storing lanes and the lane that takes the ticket: its write-through stores have left before
    // the ticket is taken -- no release fence, which would write back every dirty line of this L2, the gradient included)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) last = atomicAdd(ticket, 1) == chunks * B - 1;
    __syncthreads();
    if (!last) return;
    // every partial is read by a load that bypasses this CU's cache: no acquire fence either
    float mine = 0.f;
    for (int idx = t; idx < 4 * B; idx += kBlock) {       // (body, component); the stride keeps a thread on one component
        const int body = idx >> 2, k = idx & 3;
        const gfloat* p = (const gfloat*)partial + (size_t)body * chunks * 4 + k;
        float acc = 0.f;
        for (int j = 0; j < chunks; ++j) acc += __hip_atomic_load(p + 4 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            const float v = acc / wsum;
            loss[body] = v;
            mine += v;
        } else {
            g_transl[3 * body + k - 1] = acc;
        }
    }
    tree[t] = mine;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (t < h) tree[t] += tree[t + h];
        __syncthreads();
    }
    if (t == 0) { total[0] = tree[0]; *ticket = 0; }
}

// One thread per output row and body; a row's entries are added in CSR order in float32.
__global__ __launch_bounds__(kBlock) void mesh_transfer_kernel(
    const int* __restrict__ indptr, const int* __restrict__ indices, const float* __restrict__ data,
    const float* __restrict__ src, int R, int N, float* __restrict__ out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, b = blockIdx.y;
    if (i >= R) return;
    const float* s = src + (size_t)b * N * 3;
    float x = 0.f, y = 0.f, z = 0.f;
    for (int k = indptr[i], e = indptr[i + 1]; k < e; ++k) {
        const float w = data[k];
        const float* p = s + (size_t)indices[k] * 3;
        x = __builtin_fmaf(w, p[0], x); y = __builtin_fmaf(w, p[1], y); z = __builtin_fmaf(w, p[2], z);
    }
    float* o = out + ((size_t)b * R + i) * 3;
    o[0] = x; o[1] = y; o[2] = z;
}

}  // namespace

extern "C" size_t tuch_vertex_fit_scratch_floats(int B, int V)
{
    if (B <= 0 || V <= 0) return 0;
    return (size_t)B * ceil_div(V, kChunk) * 4;
}

extern "C" int tuch_vertex_fit_terms(const float* verts, const float* transl, const float* target, const float* weights,
                                     int B, int V, float weight_sum, float* scratch, int* ticket, float* loss,
                                     float* total, float* grad_verts, float* grad_transl, void* stream)
{
    TUCH_REQUIRE(verts && transl && target && scratch && ticket && loss && total && grad_verts && grad_transl,
                 "tuch_vertex_fit_terms: null pointer");
    TUCH_REQUIRE(B > 0 && B <= 65535 && V > 0 && V <= (1 << 30) && (long long)B * ceil_div(V, kChunk) < (1ll << 30),
                 "tuch_vertex_fit_terms: bad sizes");
    TUCH_REQUIRE(weight_sum != 0.f && weight_sum == weight_sum, "tuch_vertex_fit_terms: the weights sum to zero");
    hipLaunchKernelGGL(weights ? vertex_fit_kernel<true> : vertex_fit_kernel<false>, dim3(ceil_div(V, kChunk), B),
                       dim3(kBlock), 0, (hipStream_t)stream, verts, transl, target, weights, B, V, weight_sum, scratch, ticket,
                       loss, total, grad_verts, grad_transl);
    return tuch_check_launch("tuch_vertex_fit_terms");
}

extern "C" int tuch_mesh_transfer(const int* indptr, const int* indices, const float* data, const float* src, int B,
                                  int num_rows, int num_src, float* out, void* stream)
{
    TUCH_REQUIRE(indptr && src && out, "tuch_mesh_transfer: null pointer");
    TUCH_REQUIRE(B > 0 && B <= 65535 && num_rows > 0 && num_src > 0, "tuch_mesh_transfer: bad sizes");
    hipLaunchKernelGGL(mesh_transfer_kernel, dim3(ceil_div(num_rows, kBlock), B), dim3(kBlock), 0, (hipStream_t)stream,
                       indptr, indices, data, src, num_rows, num_src, out);
    return tuch_check_launch("tuch_mesh_transfer");
}
