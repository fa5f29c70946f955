// The device pieces that the fit terms share: scan_term_kernel (scan_fit.hip), pc_fit_kernel (point_cloud.hip) and, for
// the corner scatter, cp_bwd_kernel (closest_point.hip).  Each is one fixed sequence of float32 operations, so a term
// gives the same bits alone or in a batch, on every call, in either mode of tuch_set_deterministic.  The two term
// kernels run workgroups of kFitBlock threads on a (chunks, B) grid.  vertex_fit_kernel (mesh_fit.hip) hands its sums
// over in the same way, with 4-float partials and a tail of its own (the reason is there).
#pragma once
#include "common.h"

constexpr int kFitBlock = 256;           // four wavefronts
constexpr int kFitWaves = kFitBlock / 64;
constexpr int kFitPart = 8;              // floats per partial: sum w rho, grad_transl.xyz, the normaliser, 3 unused

typedef __attribute__((address_space(1))) float gfloat;

// rho of tuch_scan_fit_terms and tuch_point_cloud_fit_terms, as include/tuch_amd.h numbers them
enum { TUCH_SCAN_RHO_SQUARED = 0, TUCH_SCAN_RHO_DISTANCE = 1, TUCH_SCAN_RHO_GMOF = 2 };

// rho(d2) and its derivative.  'distance' has derivative 0 at d2 = 0 (vertex_fit's convention: torch.norm's subgradient).
static __device__ __forceinline__ void fit_rho(int rho, float sigma2, float d2, float& value, float& slope)
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

// rows of a face's corners vi[k] (of the body whose row 0 is `body_row`) += -bw[k] (ex, ey, ez): 64-bit fixed-point
// integer atomics (kFixed, deterministic mode) or float atomics
template <bool kFixed>
static __device__ __forceinline__ void fit_scatter_corners(float* __restrict__ grad_verts, long long* __restrict__ grad_fixed,
                                                           size_t body_row, const int (&vi)[3], const float (&bw)[3],
                                                           float ex, float ey, float ez)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t row = (body_row + vi[k]) * 3;
        if (kFixed) {
            fixed_add(grad_fixed + row, -bw[k] * ex);
            fixed_add(grad_fixed + row + 1, -bw[k] * ey);
            fixed_add(grad_fixed + row + 2, -bw[k] * ez);
        } else {
            atomicAdd(grad_verts + row, -bw[k] * ex);
            atomicAdd(grad_verts + row + 1, -bw[k] * ey);
            atomicAdd(grad_verts + row + 2, -bw[k] * ez);
        }
    }
}

struct FitShared {
    float red[kFitWaves][4];
    float wsum;
    float tree[kFitBlock];
    bool last;
};

// The normaliser of a body, get(0) + .. + get(count - 1) in one fixed order (a thread's elements, its wavefront, the
// wavefronts): every workgroup of the body gets the same bits, alone or in a batch.  Called by the whole workgroup.
template <typename Get>
static __device__ __forceinline__ float fit_body_sum(FitShared& sh, int count, Get get)
{
    const int t = threadIdx.x;
    float acc = 0.0f;
    for (int i = t; i < count; i += kFitBlock) acc += get(i);
    acc = wave_sum_lane0(acc);
    if ((t & 63) == 0) sh.red[t >> 6][0] = acc;
    __syncthreads();
    if (t == 0) {
        float a = sh.red[0][0];
#pragma unroll
        for (int j = 1; j < kFitWaves; ++j) a += sh.red[j][0];
        sh.wsum = a;
    }
    __syncthreads();
    const float wsum = sh.wsum;
    __syncthreads();                                          // (red is written again by the tail)
    return wsum;
}

// The tail of a term kernel, called by every thread of every workgroup (c, b) = blockIdx.xy with the thread's share of
// the loss numerator s and of grad_transl (gx, gy, gz), and the body's normaliser n.  partial: [B][chunks][kFitPart]
// floats; *ticket: zero before the launch, left zero.  The workgroup that arrives last writes
//   per_body[b] = n_b != 0 ? scale (sum_c s / n_b) : 0,  grad_transl[b] = sum_c g,  total[0] = sum_b per_body[b]:
// every body's chunks in chunk order, the bodies in a fixed tree -- no float atomics.
//
// The hand-over (the drain form).  The five partial sums of a workgroup are stored by lanes 0 .. 4 of wavefront 0 as
// relaxed agent-scope stores: write-through, they go past this XCD's L2, which other XCDs do not read.  s_waitcnt
// vmcnt(0) returns once every store of THAT wavefront has been acknowledged, and only then does its lane 0 take the
// ticket (a relaxed agent-scope atomic, performed where every XCD sees it).  So a workgroup that has been counted has
// its partial in memory, and the one that counts chunks * B - 1 others before it finds them all there.  The storing
// lanes and the ticket lane must share a wavefront because vmcnt is a counter of the wavefront: the wait covers no
// other wavefront's stores, and a barrier orders execution, not the arrival of stores.  The last workgroup reads
// behind its barrier, which lane 0 reaches only with the ticket's value in hand, and with relaxed agent-scope loads,
// which bypass this CU's cache and the L2 lines that are not coherent: nothing stale can be hit.  No release fence,
// which would write back every dirty line of this L2 -- the gradient rows just written among them -- and no acquire
// fence, which would invalidate caches that these loads do not use (vertex_fit_kernel at batch 64: 19.9 us with the
// fences, 11.0 us without).  The ticket's reset is ordered before the next launch by the end of this one.
static __device__ __forceinline__ void fit_reduce_tail(FitShared& sh, float s, float gx, float gy, float gz, float n,
                                                       float scale, float* partial, int* ticket, int B,
                                                       float* __restrict__ per_body, float* __restrict__ total,
                                                       float* __restrict__ grad_transl)
{
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x, chunks = gridDim.x;
    s = wave_sum_lane0(s); gx = wave_sum_lane0(gx); gy = wave_sum_lane0(gy); gz = wave_sum_lane0(gz);
    if ((t & 63) == 0) {
        float* r = sh.red[t >> 6];
        r[0] = s; r[1] = gx; r[2] = gy; r[3] = gz;
    }
    __syncthreads();
    if (t < 5) {
        float acc = n;
        if (t < 4) {
            acc = sh.red[0][t];
#pragma unroll
            for (int j = 1; j < kFitWaves; ++j) acc += sh.red[j][t];
        }
        __hip_atomic_store((gfloat*)partial + ((size_t)b * chunks + c) * kFitPart + t, acc, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) sh.last = atomicAdd(ticket, 1) == chunks * B - 1;
    __syncthreads();
    if (!sh.last) return;
    float mine = 0.0f;
    for (int idx = t; idx < 4 * B; idx += kFitBlock) {        // (body, component); the stride keeps a thread on one component
        const int body = idx >> 2, k = idx & 3;
        const gfloat* p = (const gfloat*)partial + (size_t)body * chunks * kFitPart;
        float acc = 0.0f;
        for (int j = 0; j < chunks; ++j)
            acc += __hip_atomic_load(p + kFitPart * j + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            const float nb = __hip_atomic_load(p + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float value = nb != 0.0f ? scale * (acc / nb) : 0.0f;
            per_body[body] = value;
            mine += value;
        } else {
            grad_transl[3 * body + k - 1] = acc;
        }
    }
    sh.tree[t] = mine;
    __syncthreads();
    for (int h = kFitBlock / 2; h > 0; h >>= 1) {
        if (t < h) sh.tree[t] += sh.tree[t + h];
        __syncthreads();
    }
    if (t == 0) {
        total[0] = sh.tree[0];
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
