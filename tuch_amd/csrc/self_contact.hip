// Self-contact detection: which vertices of a body touch, and which body regions do they join.
//
// Replaces TUCH.get_verts_in_contact, tuch/train/train_module.py:93-110, which materialises the [V,V] squared-distance
// matrix per body in a Python loop, thresholds it (`< euclthres**2`), multiplies by the geodesic mask and takes a row
// minimum; and produces the contact signature (minimum distance per pair of body regions) whose per-body minimum
// eval.py:135-136 reads from a file.
//
// Vertex i is in contact with j when mask[i][j] and |v_i - v_j|^2 < euclthres^2.  One pass over the pairs:
//   * a workgroup of 256 threads owns one body and 256 rows i (one per lane) and walks ALL columns j, so every
//     per-vertex result has one owner: no merge, no workspace;
//   * columns are staged 1024 at a time as x / y / z in LDS (the next tile's global loads are in flight while the
//     current one is used) and read four at a time at wave-uniform addresses (b128 broadcasts);
//   * the lane's mask word for the 64 columns of a step is ONE 64-bit load, bits[step][i] in the layout of
//     tuch_pack_geomask: adjacent lanes read adjacent words; the next step's word is requested a step ahead;
//   * the distance test runs first and without the mask: a step costs the seven vector operations per pair of the
//     distance and a running minimum.  Only when some lane of the wavefront has a column within the threshold AND a
//     non-zero mask word is the step looked at again, four columns at a time, and only the groups of four with a
//     qualifying pair reach the per-pair code.  Qualifying pairs are rare (a few hundred of 47 million per body), mesh
//     neighbours -- close but masked out -- are what the second look is mostly spent on;
//   * a qualifying pair updates the lane's (minimum, partner) -- columns ascend and the comparison is strict, so the
//     partner is the smallest j among equal minima -- and, with a region table, the signature entries (r1, r2) of the
//     two vertices' region lists with an unsigned-integer atomic minimum on the float's bit pattern (non-negative
//     floats order like their bits): associative and commutative, so the result does not depend on the order of
//     arrival or on the batch.  The atomics go to global memory directly: per body there are hundreds of them, far
//     fewer than the R^2 entries a per-workgroup table in LDS would have to be cleared and flushed for, and the
//     kernel keeps its 12 KiB of LDS per workgroup whatever R is.  An entry that is already small enough is not
//     touched (plain read first), which is what keeps a call where everything qualifies from serialising;
//   * the body's minimum (cnc) is the minimum over the wavefronts' lanes, one atomic per wavefront that found contact.
// Squared distances are direct differences, evaluated as v2v.hip and region_min.hip do: the same bits.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 1024;                 // columns staged per pass (12 KiB of LDS)
constexpr int kStage = kTile / kBlock;      // columns a thread stages per tile
constexpr int kMaxRegions = 128;

__global__ __launch_bounds__(kBlock) void self_contact_init_kernel(float* __restrict__ sig, size_t n_sig,
                                                                  float* __restrict__ cnc, int B)
{
    const float inf = __builtin_inff();
    const size_t n = n_sig + (size_t)B, stride = (size_t)gridDim.x * kBlock;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        if (k < n_sig) sig[k] = inf; else cnc[k - n_sig] = inf;
    }
}

__device__ __forceinline__ float dist2(float px, float py, float pz, float x, float y, float z)
{
    const float dx = px - x, dy = py - y, dz = pz - z;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

template <bool kRegions>
__global__ __launch_bounds__(kBlock) void self_contact_kernel(
    const float* __restrict__ verts,          // [B,V,3]
    const uint64_t* __restrict__ bits,        // [W][V]: bit k of bits[w][i] = mask[i][64 w + k]
    int V, float e2,
    const int32_t* __restrict__ vreg_off,     // [V+1]   (kRegions)
    const int32_t* __restrict__ vreg, int R,
    uint8_t* __restrict__ in_contact, int32_t* __restrict__ partner, float* __restrict__ min_d2,   // [B,V]
    unsigned int* sig,                        // [B,R,R] bit patterns, preset to +inf (kRegions)
    unsigned int* cnc)                        // [B], preset to +inf
{
    __shared__ __attribute__((aligned(16))) float sx[kTile], sy[kTile], sz[kTile];
    // body index fastest in the launch order, as in v2v.hip (XCD b % 8 keeps body b's vertices in one L2)
    const int b = blockIdx.x;
    const int i = blockIdx.y * kBlock + threadIdx.x;
    const bool live = i < V;
    const float* vb = verts + (size_t)b * V * 3;
    const int ic = live ? i : V - 1;
    const float px = vb[3 * ic], py = vb[3 * ic + 1], pz = vb[3 * ic + 2];
    const int nsteps = (V + 63) >> 6;
    const float inf = __builtin_inff();
    float best = inf;
    int part = -1;
    int a_beg = 0, a_end = 0;
    if (kRegions && live) { a_beg = vreg_off[i]; a_end = vreg_off[i + 1]; }

    // a qualifying pair (this lane's row i, column j): rare, so nothing here is tuned -- it only has to be right
    auto hit = [&](int j, float d) {
        if (d < best) { best = d; part = j; }
        if (kRegions) {
            const unsigned int key = __float_as_uint(d);
            const int c_beg = vreg_off[j], c_end = vreg_off[j + 1];
            for (int a = a_beg; a < a_end; ++a) {
                const int r1 = vreg[a];
                if ((unsigned int)r1 >= (unsigned int)R) continue;
                unsigned int* row = sig + ((size_t)b * R + r1) * R;
                for (int c = c_beg; c < c_end; ++c) {
                    const int r2 = vreg[c];
                    if ((unsigned int)r2 >= (unsigned int)R) continue;
                    // entries only ever decrease: a stale read can only cause a redundant atomic
                    if (__hip_atomic_load(row + r2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(row + r2, key);
                }
            }
        }
    };

    float c[kStage][3];                       // the next tile's columns, on their way while the current tile is used
    auto fetch = [&](int t0) {
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int j = min(t0 + (int)threadIdx.x + kBlock * u, V - 1);      // past V: copies of the last vertex
            c[u][0] = vb[3 * j]; c[u][1] = vb[3 * j + 1]; c[u][2] = vb[3 * j + 2];
        }
    };
    fetch(0);
    uint64_t next_word = live ? bits[i] : 0ull;                                // rows past V never qualify
    for (int t0 = 0; t0 < V; t0 += kTile) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int k = threadIdx.x + kBlock * u;
            sx[k] = c[u][0]; sy[k] = c[u][1]; sz[k] = c[u][2];
        }
        __syncthreads();
        if (t0 + kTile < V) fetch(t0 + kTile);
        const int tn = min(kTile, V - t0);
        for (int g = 0; g < tn; g += 64) {
            const int w = (t0 + g) >> 6;
            uint64_t word = next_word;
            if (w + 1 < nsteps) next_word = live ? bits[(size_t)(w + 1) * V + i] : 0ull;
            if (tn - g < 64) word &= (1ull << (tn - g)) - 1ull;                // columns past V never qualify
            // all 64 columns of the step, unmasked (the whole tile is staged, columns past V included)
            float m = inf;
#pragma unroll
            for (int kk = 0; kk < 64; kk += 4) {
                const float4 x4 = *(const float4*)&sx[g + kk];
                const float4 y4 = *(const float4*)&sy[g + kk];
                const float4 z4 = *(const float4*)&sz[g + kk];
                const float d0 = dist2(px, py, pz, x4.x, y4.x, z4.x), d1 = dist2(px, py, pz, x4.y, y4.y, z4.y);
                const float d2 = dist2(px, py, pz, x4.z, y4.z, z4.z), d3 = dist2(px, py, pz, x4.w, y4.w, z4.w);
                m = fminf(fminf(m, d0), fminf(fminf(d1, d2), d3));
            }
            if (__builtin_amdgcn_ballot_w64(m < e2 && word != 0ull) == 0ull) continue;      // wave-uniform
            for (int kk = 0; kk < 64; kk += 4) {
                const float4 x4 = *(const float4*)&sx[g + kk];
                const float4 y4 = *(const float4*)&sy[g + kk];
                const float4 z4 = *(const float4*)&sz[g + kk];
                const float d[4] = {dist2(px, py, pz, x4.x, y4.x, z4.x), dist2(px, py, pz, x4.y, y4.y, z4.y),
                                    dist2(px, py, pz, x4.z, y4.z, z4.z), dist2(px, py, pz, x4.w, y4.w, z4.w)};
                const unsigned int nib = (unsigned int)(word >> kk) & 15u;
                bool q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) q[u] = d[u] < e2 && ((nib >> u) & 1u);
                if (__builtin_amdgcn_ballot_w64(q[0] || q[1] || q[2] || q[3]) == 0ull) continue;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (q[u]) hit(t0 + g + kk + u, d[u]);
            }
        }
    }
    if (live) {
        const size_t o = (size_t)b * V + i;
        in_contact[o] = part >= 0;
        partner[o] = part;
        min_d2[o] = best;
    }
    const float wave_best = wave_min_uniform(best);
    if ((threadIdx.x & 63) == 0 && wave_best < inf) atomicMin(cnc + b, __float_as_uint(wave_best));
}

}  // namespace

extern "C" int tuch_self_contact(const float* verts, const uint64_t* geomask_bits, int B, int V, float euclthres,
                                 const int32_t* vreg_off, const int32_t* vreg, int R, uint8_t* in_contact,
                                 int32_t* partner, float* min_d2, float* sig_d2, float* cnc_d2, void* stream)
{
    TUCH_REQUIRE(B >= 0, "tuch_self_contact: bad batch %d", B);
    if (B == 0) return TUCH_OK;
    TUCH_REQUIRE(verts && geomask_bits && in_contact && partner && min_d2 && cnc_d2, "tuch_self_contact: null pointer");
    TUCH_REQUIRE(V >= 1 && V <= 65535 * kBlock, "tuch_self_contact: bad vertex count %d", V);
    const bool regions = vreg_off != nullptr;
    if (regions) {
        TUCH_REQUIRE(vreg && sig_d2, "tuch_self_contact: a region table needs vreg and sig_d2");
        TUCH_REQUIRE(R >= 1 && R <= kMaxRegions, "tuch_self_contact: %d regions, 1 to %d are supported", R, kMaxRegions);
    }
    hipStream_t s = (hipStream_t)stream;
    const float e2 = euclthres > 0.0f ? euclthres * euclthres : 0.0f;          // d2 < 0 never holds: nothing qualifies
    const size_t n_sig = regions ? (size_t)B * R * R : 0;
    const size_t n_init = n_sig + (size_t)B;
    const int init_blocks = (int)((n_init + kBlock - 1) / kBlock < 2048 ? (n_init + kBlock - 1) / kBlock : 2048);
    hipLaunchKernelGGL(self_contact_init_kernel, dim3(init_blocks), dim3(kBlock), 0, s, regions ? sig_d2 : nullptr, n_sig,
                       cnc_d2, B);
    const dim3 grid(B, ceil_div(V, kBlock));
    if (regions)
        hipLaunchKernelGGL(self_contact_kernel<true>, grid, dim3(kBlock), 0, s, verts, geomask_bits, V, e2, vreg_off, vreg, R,
                           in_contact, partner, min_d2, (unsigned int*)sig_d2, (unsigned int*)cnc_d2);
    else
        hipLaunchKernelGGL(self_contact_kernel<false>, grid, dim3(kBlock), 0, s, verts, geomask_bits, V, e2,
                           (const int32_t*)nullptr, (const int32_t*)nullptr, 0, in_contact, partner, min_d2,
                           (unsigned int*)nullptr, (unsigned int*)cnc_d2);
    return tuch_check_launch("tuch_self_contact");
}
