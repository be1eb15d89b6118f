// ransac_common.h -- what the two RANSAC verifiers (homography_kernels.hip; fundamental_kernels.hip, S18) share:
// the by-value job table, the gather kernel, the counter-based random source, the fixed-order block and partial sums, the argmax
// over hypothesis counts and the Hartley normalisation of the winner's inliers.  Included by both files; every definition lives
// in an unnamed namespace, so each translation unit carries its own copy of the gather kernel.
#pragma once

#include "efx_device.h"
#include "../../include/efx.h"

#include <stdint.h>

namespace {

#define HOM_RB 256           // threads of the row-pass and finish workgroups; a row-pass workgroup owns 256 rows

struct RansacJobs {                                // a chain's pairs, passed by value
    const uint32_t* kq[EFX_MAX_BATCH];             // LOCATION row (short2 bits) of the query / train keypoint matrix
    const uint32_t* kt[EFX_MAX_BATCH];
    const int* m[EFX_MAX_BATCH];                   // {queryIdx, trainIdx, distance} rows
    const int* nm[EFX_MAX_BATCH];                  // device count (NULL: the capacity)
    void* res[EFX_MAX_BATCH];                      // efx_homography / efx_fundamental (one layout)
    uint8_t* mask[EFX_MAX_BATCH];
    unsigned long long seed;
    int q_cap, t_cap, cap, hyps, refine;
    float thr;
};

__device__ __forceinline__ float hom_nan() { return __builtin_nanf(""); }

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- kernel 1: gather ----
__global__ __launch_bounds__(256) void hom_gather_kernel(RansacJobs J, float4* __restrict__ pts, int* __restrict__ nrow)
{
    const int p = blockIdx.z;
    const int* cp = J.nm[p];
    int n = J.cap;
    if (cp) { n = *cp; n = n < 0 ? 0 : (n > J.cap ? J.cap : n); }
    if (blockIdx.x == 0 && threadIdx.x == 0) nrow[p] = n;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int* row = J.m[p] + 3 * (size_t)k;
    const int qi = row[0], ti = row[1];
    float4 v = make_float4(hom_nan(), hom_nan(), hom_nan(), hom_nan());
    if (qi >= 0 && qi < J.q_cap && ti >= 0 && ti < J.t_cap) {
        const uint32_t a = J.kq[p][qi], b = J.kt[p][ti];
        v = make_float4((float)(short)(a & 0xFFFFu), (float)(short)(a >> 16), (float)(short)(b & 0xFFFFu), (float)(short)(b >> 16));
    }
    pts[(size_t)p * J.cap + k] = v;
}

// ---- the winner and the refit: row passes over a grid, then one workgroup per pair ----
// Every row-pass workgroup writes its partial sums to scratch; a later kernel adds them in workgroup order (thread t takes partials
// t, t + 256, ..., then a fixed reduction tree), so every sum has one order whatever the pair's place in a batch.

__device__ __forceinline__ long long block_sum_ll(long long v, long long* s_ll)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) s_ll[wave] = v;
    __syncthreads();
    return s_ll[0] + s_ll[1] + s_ll[2] + s_ll[3];
}

template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*s_red)[HOM_RB / 64])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) s_red[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ((s_red[k][0] + s_red[k][1]) + s_red[k][2]) + s_red[k][3];
}

// the partials of pair p (K per workgroup, nblk workgroups) summed in workgroup order
template <int K>
__device__ __forceinline__ void partial_sum(const double* __restrict__ part, int p, int nblk, double (&v)[K], double (*s_red)[HOM_RB / 64])
{
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = 0.0;
    for (int b = threadIdx.x; b < nblk; b += HOM_RB) {
#pragma unroll
        for (int k = 0; k < K; k++) v[k] += part[((size_t)p * nblk + b) * K + k];
    }
    block_sum<K>(v, s_red);
}

// centroids of the winner's inliers (exact integer sums) -> cx / cy of src and dst
__device__ __forceinline__ void hom_centroids(const long long* __restrict__ pa, int p, int nblk, double cnt, double* cxy, long long* s_ll)
{
    long long v[4] = { 0, 0, 0, 0 };
    for (int b = threadIdx.x; b < nblk; b += HOM_RB) {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] += pa[((size_t)p * nblk + b) * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) cxy[k] = (double)block_sum_ll(v[k], s_ll) / cnt;
}

// S16 step 6, by every workgroup that needs it: the most inliers, ties to the lowest index (each thread scans ascending indices
// with a strict >); nv = the number of valid hypotheses
__device__ __forceinline__ void hom_argmax(const int* __restrict__ K, int hyps, int& best, int& bi, int& nv, int* s_i)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    best = -1; bi = 0x7fffffff; nv = 0;
    for (int h = tid; h < hyps; h += HOM_RB) {
        const int c = K[h];
        if (c >= 0) { nv++; if (c > best) { best = c; bi = h; } }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o, 64), oi = __shfl_xor(bi, o, 64);
        nv += __shfl_xor(nv, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_i[wave] = best; s_i[4 + wave] = bi; s_i[8 + wave] = nv; }
    __syncthreads();
    best = -1; bi = 0x7fffffff; nv = 0;
    for (int w = 0; w < 4; w++) {
        nv += s_i[8 + w];
        if (s_i[w] > best || (s_i[w] == best && s_i[4 + w] < bi)) { best = s_i[w]; bi = s_i[4 + w]; }
    }
}

// the Hartley normalisation of both sides: centroids c[0..3] (src x, y, dst x, y) and scales ss, sd = sqrt(2) / mean distance
__device__ __forceinline__ void hom_hartley(const long long* __restrict__ pa, const double* __restrict__ pb, int p, int nblk, int best,
                                            double* c, double& ss, double& sd, long long* s_ll, double (*s_red)[HOM_RB / 64])
{
    const double cnt_d = (double)best;
    hom_centroids(pa, p, nblk, cnt_d, c, s_ll);
    double d[2];
    partial_sum<2>(pb, p, nblk, d, s_red);
    ss = 1.4142135623730951 / (d[0] / cnt_d);
    sd = 1.4142135623730951 / (d[1] / cnt_d);
}

} // namespace
