// match_kernels.hip -- brute-force Hamming matcher on the device (the consumer of the descriptors).
// Semantics of cv::BFMatcher(NORM_HAMMING) as the reference's samples use it:
//   knnMatch(query, train, k = 2)          samples/sample_image_sequence.cpp:81, 114-115
//   match() with crossCheck = true         samples/sample_feature_matching.cpp:99-101
// Distance = number of differing bits; ties are resolved towards the lower train index (the order in which a
// sequential scan with a strict `<` meets them).
//
// One search family serves every entry point.  A launch runs a table of jobs (KnnJobs, job z = blockIdx.z): knnMatch is one
// job, crossCheck two knnMatch runs, mutual matching both directions of up to EFX_MAX_BATCH pairs.  Row counts are read at
// kernel start from device ints (NULL: the capacity -- what the host-count calls pass), grids are sized from the capacities,
// and workgroups past a count exit at once.  The train set of a job is split into chunks along grid.y for occupancy; a merge
// kernel turns the per-chunk best two into the public knnMatch lists (idx / dist, n x 2 int32, -1 where missing).
//   small sets: knn2_dc_kernel -- one lane owns one query descriptor (8 or 16 dwords in VGPRs); the train descriptors are read
//     through the scalar cache (the address is wave-uniform, so every lane xors against SGPR operands) and each 32-bit word
//     costs one v_xor + one v_bcnt_u32 (popcount with accumulate);
//   large sets: expand_dc_kernel, then knn2_mfma_kernel -- the distance matrix as a GEMM on the matrix cores.

#include <atomic>
#include "efx_device.h"
#include <stdlib.h>
#include <type_traits>

namespace {

struct Best2 { int d0, i0, d1, i1; };

struct KnnJobs {                         // a launch's jobs, passed by value (kernel arguments: no table upload, nothing to race)
    const uint8_t* q[EFX_MAX_BATCH];     // query rows of pair p: raw descriptors (popcount path) or expanded rows (matrix cores)
    const uint8_t* t[EFX_MAX_BATCH];     // train rows of pair p
    const int* nq[EFX_MAX_BATCH];        // device counts (NULL: the capacity), clamped to [0, capacity]
    const int* nt[EFX_MAX_BATCH];
    int* out[EFX_MAX_BATCH];             // mutual matching: d_matches (3 ints per row) and d_nmatches of pair p
    int* nout[EFX_MAX_BATCH];
    int* idx;                            // the knnMatch lists of job z: 2 ints per query from idx / dist + 2 * cap * z
    int* dist;
    size_t q_pitch, t_pitch;             // row pitches of the rows above
    int q_cap, t_cap;                    // capacities
    int cap;                             // row stride of the partial and knnMatch lists: >= the query capacity of every job
    int nchunks;                         // train chunks per job (grid.y)
};

__device__ __forceinline__ int knn_count(const int* p, int cap)
{
    if (!p) return cap;
    const int n = *p;
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// the operands of job z: pair z >> 1 in direction z & 1 (0: query -> train, 1: train -> query)
struct KnnJob { const uint8_t* q; const uint8_t* t; size_t qp, tp; int nq, nt; };
__device__ __forceinline__ KnnJob knn_job(const KnnJobs& J, int z)
{
    const int p = z >> 1;
    const int na = knn_count(J.nq[p], J.q_cap), nb = knn_count(J.nt[p], J.t_cap);
    KnnJob j;
    if (z & 1) { j.q = J.t[p]; j.t = J.q[p]; j.qp = J.t_pitch; j.tp = J.q_pitch; j.nq = nb; j.nt = na; }
    else { j.q = J.q[p]; j.t = J.t[p]; j.qp = J.q_pitch; j.tp = J.t_pitch; j.nq = na; j.nt = nb; }
    return j;
}

// popcount search: the trains of job z in nchunks chunks of ceil(nt / nchunks)
template <int NW>   // dwords per descriptor: 8 (256 bit) or 16 (512 bit)
__global__ __launch_bounds__(256) void knn2_dc_kernel(KnnJobs J, Best2* __restrict__ partial)
{
    const int z = blockIdx.z;
    const KnnJob j = knn_job(J, z);
    if ((int)blockIdx.x * 256 >= j.nq) return;
    const int qi = blockIdx.x * 256 + threadIdx.x;
    const int chunk = (j.nt + J.nchunks - 1) / J.nchunks;
    const int t0 = blockIdx.y * chunk, t1 = min(t0 + chunk, j.nt);
    uint32_t q[NW];
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(j.q + (size_t)min(qi, j.nq - 1) * j.qp);
#pragma unroll
    for (int k = 0; k < NW; k++) q[k] = qp[k];
    Best2 b; b.d0 = 0x7fffffff; b.i0 = -1; b.d1 = 0x7fffffff; b.i1 = -1;
    for (int t = t0; t < t1; t++) {
        const uint32_t* tp = reinterpret_cast<const uint32_t*>(j.t + (size_t)t * j.tp);   // wave-uniform
        int d = 0;
#pragma unroll
        for (int k = 0; k < NW; k++) d += __popc(q[k] ^ tp[k]);
        if (d < b.d0) { b.d1 = b.d0; b.i1 = b.i0; b.d0 = d; b.i0 = t; }
        else if (d < b.d1) { b.d1 = d; b.i1 = t; }
    }
    if (qi < j.nq) partial[((size_t)z * J.nchunks + blockIdx.y) * J.cap + qi] = b;
}

// the chunks' best two of job z -> its knnMatch lists
__global__ __launch_bounds__(256) void knn2_merge_dc_kernel(KnnJobs J, const Best2* __restrict__ partial)
{
    const int z = blockIdx.z;
    const KnnJob j = knn_job(J, z);
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= j.nq) return;
    Best2 b; b.d0 = 0x7fffffff; b.i0 = -1; b.d1 = 0x7fffffff; b.i1 = -1;
    // chunks are visited in train order and candidates inside a chunk are already ordered, so a strict `<`
    // keeps the lower train index on ties
    for (int c = 0; c < J.nchunks; c++) {
        const Best2 p = partial[((size_t)z * J.nchunks + c) * J.cap + qi];
        const int cd[2] = { p.d0, p.d1 }, ci[2] = { p.i0, p.i1 };
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (ci[k] < 0) continue;
            if (cd[k] < b.d0) { b.d1 = b.d0; b.i1 = b.i0; b.d0 = cd[k]; b.i0 = ci[k]; }
            else if (cd[k] < b.d1) { b.d1 = cd[k]; b.i1 = ci[k]; }
        }
    }
    const size_t r = 2 * ((size_t)z * J.cap + qi);
    J.idx[r] = b.i0; J.idx[r + 1] = b.i1;
    J.dist[r] = b.i0 >= 0 ? b.d0 : -1; J.dist[r + 1] = b.i1 >= 0 ? b.d1 : -1;
}

// ================================================================================================
// The same search on the matrix cores (large query / train sets).  With every bit expanded to a byte of +-1, the dot product of
// two descriptors is nbits - 2 * hamming: the brute-force distance matrix is an int8 GEMM, exact in the i32 accumulator, and
// v_mfma_i32_32x32x32_i8 does 32 x 32 x 32 of its terms per instruction (the popcount kernel above spends 2 VALU instructions
// per 32 bit-pairs of ONE query).  Layout: the TRAINS are the M operand (32-row tiles staged in LDS per workgroup step, shared by
// the eight waves), the QUERIES the N operand (32 per wave, kept in registers for the wave's life), so that a lane of the C tile
// holds 16 trains of ONE query and keeps that query's best two in registers: no cross-lane traffic until the two row-halves of a
// query are merged at the very end.  A tile whose maximum does not beat any lane's second best (almost all of them, after the
// first few) is dismissed with 8 v_max3 per lane.
// ================================================================================================
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ExpandJobs {                      // the descriptor matrices of one expansion launch (matrix = blockIdx.z)
    const uint8_t* src[2 * EFX_MAX_BATCH];
    const int* n[2 * EFX_MAX_BATCH];
    size_t pitch[2 * EFX_MAX_BATCH];
    uint8_t* dst[2 * EFX_MAX_BATCH];     // its slot: room for round_up(capacity, 256) expanded rows
    int cap[2 * EFX_MAX_BATCH];
};

// bits -> matrix-core operands, matrix z -> its slot E.dst[z]: int8 bytes of +1 / -1, or FP4 (E2M1) nibbles of +1.0 (0x2) /
// -1.0 (0xA), two per byte (round 4).  Bit j of a descriptor -> element j (the order only has to be the same for queries and
// trains).  Rows [0, n) expanded, [n, n rounded up to 256) zero (they contribute nothing to a dot product; padded trains are
// masked by index): a query block reads whole 256-row blocks, a train step whole 32-row tiles.  The rest is never read and not
// written.  ONE expansion serves a matrix as the query operand of one direction and the train operand of the other.
template <bool FP4>
__global__ __launch_bounds__(256) void expand_dc_kernel(ExpandJobs E, int nbytes)
{
    const int z = blockIdx.z;
    const int n = knn_count(E.n[z], E.cap[z]);
    const int groups = nbytes >> 1;                        // 16 bits per thread
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)((n + 255) & ~255) * groups) return;
    const int row = (int)(i / groups), g = (int)(i - (size_t)row * groups);
    uint8_t* __restrict__ d = E.dst[z];
    const uint8_t* p = E.src[z] + (size_t)row * E.pitch[z] + 2 * g;
    if constexpr (FP4) {
        uint2 out = make_uint2(0u, 0u);
        if (row < n) {
            uint32_t w[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                uint32_t x = p[k];                          // bit j -> bit 4 j
                x = (x | (x << 12)) & 0x000f000fu;
                x = (x | (x << 6)) & 0x03030303u;
                x = (x | (x << 3)) & 0x11111111u;
                w[k] = 0x22222222u | ((~x & 0x11111111u) << 3);  // 1 -> 0x2 (+1.0), 0 -> 0xA (-1.0)
            }
            out = make_uint2(w[0], w[1]);
        }
        *reinterpret_cast<uint2*>(d + ((size_t)row * groups + g) * 8) = out;
    } else {
        uint4 out = make_uint4(0u, 0u, 0u, 0u);
        if (row < n) {
            const uint32_t bits = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t ones = (((bits >> (4 * k)) & 15u) * 0x00204081u) & 0x01010101u;   // bit -> 0 / 1 per byte
                w[k] = ones | ((ones ^ 0x01010101u) * 0xffu);                                     // 1 -> 0x01, 0 -> 0xff
            }
            out = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(d + ((size_t)row * groups + g) * 16) = out;
    }
}

// (dot product, train index) a better than b: larger dot (smaller distance), then lower index
// The best-two bookkeeping compares INTEGER keys.  The int8 kernel's accumulators are integers already; the FP4 kernel's fp32
// accumulators start at KNN_FP4_BIAS instead of 0, so that every value is a positive float (a dot product is within +-512, and
// exact), and positive floats order like their bit patterns.  Integer max / compare have no NaN cases to canonicalise
// (fmaxf costs a v_max_f32 x, x per operand), and -- unlike an inline-asm v_max3_f32, round 4's first form of the group
// filter -- they are instructions the compiler knows read the MFMA's result registers: it places the wait states behind the
// last MFMA itself (the asm form read stale accumulators and lost ~1 in 300 best-two updates on tie-heavy sets:
// tools/microbench/match_fuzz.py found it, the parity tests' random sets had not).
#define KNN_FP4_BIAS 1024.f
__device__ __forceinline__ int knn_key(float v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ int knn_key(int v) { return v; }
__device__ __forceinline__ int knn_max4(int a, int b, int c, int d)
{
    const int ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}
template <class T> __device__ __forceinline__ bool knn_better(T da, int ia, T db, int ib) { return da > db || (da == db && (unsigned)ia < (unsigned)ib); }

// Train tiles per step.  The MX instruction halved the matrix time of a tile (8 MFMAs of 32 cycles for 512 bits), and what was
// left -- staging, barriers, the best-two bookkeeping of a tile -- then took three quarters of a step.  TT tiles share one staging
// pass and one barrier, and their TT accumulators are independent MFMA chains (a wave's MFMAs on ONE accumulator wait for each
// other).  Measured (40 000 x 40 000): a 256-bit FP4 tile is four MFMAs, two tiles amortise its barrier; a 512-bit step of two
// tiles is slower than two steps of one (0.467 against 0.436 ms: sixteen fragments up front do not fit).  int8: one tile.
constexpr int knn2_tt(int nbits, bool fp4) { return fp4 && nbits == 256 ? 2 : 1; }

// NBITS: descriptor bits (256 or 512).  Eight waves of 32 queries (two 32-query column blocks per wave read half as much LDS per
// MFMA but run at half the occupancy: 1.6 against 1.0 ms; at 512 bits FP4 180 VGPRs with spills: 0.70 ms).
// FP4 (round 4): the same GEMM on the MX matrix cores -- v_mfma_f32_32x32x64_f8f6f4 with both operands FP4 (E2M1 holds +-1.0
// exactly; no block scales: the unscaled form), 64 terms of K per instruction at the int8 instruction's issue cost (32 cycles)
// and 16 bytes per lane and operand: half the MFMAs AND half the LDS bytes per descriptor pair.  The fp32 accumulator is exact
// (|dot| <= 512).  The lane layout of the operands is the int8 form's with two elements per byte (row = lane & 31, K range by
// lane >> 5), the C layout is the shape's; which K index a nibble stands for does not matter as long as queries and trains agree.
// FP4 steps are double-buffered (round 5): two LDS copies of a step's tiles taking turns, so a step has ONE barrier (behind its
// staging stores): when a wave passes the barrier of step s + 1 every wave has finished multiplying step s, so step s + 2 may
// overwrite that copy (512 bit: 0.433 -> 0.414 ms per 40 000 x 40 000 call).  Every fragment of a step is requested up front and
// the MFMAs issue back to back as they arrive (0.425 -> 0.410 ms; 114 VGPRs at 512 bits, still four waves per SIMD; holding
// three workgroups per CU instead spills).  The int8 form keeps one tile copy (two barriers per step) and one A fragment ahead.
template <int NBITS, bool FP4>
__global__ __launch_bounds__(512) void knn2_mfma_kernel(KnnJobs J, Best2* __restrict__ partial)
{
    constexpr int TT = knn2_tt(NBITS, FP4);
    constexpr bool DB = FP4;
    constexpr int NT = 512;
    constexpr int NB = FP4 ? NBITS / 2 : NBITS;            // bytes of an expanded descriptor
    constexpr int KS = NB / 32;                            // K steps: 32 bytes of a row per MFMA (32 int8 or 64 FP4 terms)
    constexpr int LP = NB + 16;                            // LDS row pitch: rows 4 banks apart
    constexpr int NPIECE = TT * 32 * NB / 16;              // 16-byte pieces of a step's TT tiles (rows contiguous in memory)
    constexpr int NPF = (NPIECE + NT - 1) / NT;            // ... per thread
    typedef typename std::conditional<FP4, float, int>::type acc_t;
    typedef typename std::conditional<FP4, f32x16, i32x16>::type accv_t;
    const int LOWEST = FP4 ? 0 : -0x7fffffff;             // key below every real one (FP4: +0.0f)
    __shared__ __attribute__((aligned(16))) uint8_t s_tiles[(DB ? 2 : 1) * TT * 32 * LP];
    const KnnJob j = knn_job(J, blockIdx.z);
    const int nq = j.nq, nt = j.nt;
    if ((int)blockIdx.x * 256 >= nq) return;               // a workgroup past the count (uniform: before any barrier)
    const uint8_t* __restrict__ xq = j.q;
    const uint8_t* __restrict__ xt = j.t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.x * 256 + wave * 32;
    i32x4 bq[KS];
    {
        const i32x4* p = reinterpret_cast<const i32x4*>(xq + (size_t)(q0 + li) * NB + 16 * lh);
#pragma unroll
        for (int ks = 0; ks < KS; ks++) bq[ks] = p[2 * ks];
    }
    // Tiles per chunk in whole steps: a step across a chunk boundary would see trains of the next chunk twice.  The last step
    // of a job may run past its last tile into the expansion's zero rows (the count rounded up to 256)
    const int ntiles = (nt + 31) >> 5;
    const int tpc = ((ntiles + J.nchunks - 1) / J.nchunks + TT - 1) / TT * TT;
    const int tile0 = blockIdx.y * tpc, tile1 = min(tile0 + tpc, ntiles);
    int bd0 = LOWEST, bd1 = LOWEST;                        // keys (knn_key) of the best two
    int bi0 = -1, bi1 = -1;
    uint4 pf[NPF];
    auto fetch = [&](int tile) {
        const uint4* src = reinterpret_cast<const uint4*>(xt + (size_t)tile * 32 * NB);
#pragma unroll
        for (int k = 0; k < NPF; k++) if (NPIECE % NT == 0 || tid + NT * k < NPIECE) pf[k] = src[tid + NT * k];
    };
    if (tile0 < tile1) fetch(tile0);
    for (int tile = tile0; tile < tile1; tile += TT) {
        uint8_t* s_tile = s_tiles + (DB ? (((tile - tile0) / TT) & 1) * (TT * 32 * LP) : 0);
#pragma unroll
        for (int k = 0; k < NPF; k++) {
            const int piece = tid + NT * k, row = piece / (NB / 16), col = piece - row * (NB / 16);
            if (NPIECE % NT == 0 || piece < NPIECE) *reinterpret_cast<uint4*>(s_tile + row * LP + 16 * col) = pf[k];
        }
        __syncthreads();
        if (tile + TT < tile1) fetch(tile + TT);           // in flight while these tiles are multiplied
        accv_t acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; tt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[tt][r] = FP4 ? (acc_t)KNN_FP4_BIAS : (acc_t)0;
        const uint8_t* arow = s_tile + li * LP + 16 * lh;
        if constexpr (FP4) {
            i32x4 af[KS][TT];
#pragma unroll
            for (int ks = 0; ks < KS; ks++)
#pragma unroll
                for (int tt = 0; tt < TT; tt++) af[ks][tt] = *reinterpret_cast<const i32x4*>(arow + tt * 32 * LP + 32 * ks);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const i32x8 b8 = { bq[ks][0], bq[ks][1], bq[ks][2], bq[ks][3], 0, 0, 0, 0 };
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    const i32x8 a8 = { af[ks][tt][0], af[ks][tt][1], af[ks][tt][2], af[ks][tt][3], 0, 0, 0, 0 };
                    // cbsz / blgp 4: FP4 E2M1; scales 0: the unscaled form
                    acc[tt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc[tt], 4, 4, 0, 0, 0, 0);
                }
            }
        } else {
            i32x4 a = *reinterpret_cast<const i32x4*>(arow);
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const i32x4 an = *reinterpret_cast<const i32x4*>(arow + 32 * (ks + 1 < KS ? ks + 1 : ks));
                acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[ks], acc[0], 0, 0, 0);
                a = an;
            }
        }
        // C layout: column (query) = lane & 31, row (train) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5): increasing with reg
#pragma unroll
        for (int tt = 0; tt < TT; tt++) {                   // increasing train index: a strict > keeps the lower index on ties
            const int tb = (tile + tt) * 32;
            if (TT > 1 && tb >= nt) break;                  // a padding tile of the last step (wave-uniform)
            const int t0 = tb + 4 * lh;
            int key[16];
#pragma unroll
            for (int r = 0; r < 16; r++) key[r] = knn_key(acc[tt][r]);
            if (tb + 32 > nt) {                             // trains past the count must not compete
#pragma unroll
                for (int r = 0; r < 16; r++) if (t0 + (r & 3) + 8 * (r >> 2) >= nt) key[r] = LOWEST;
            }
            // A register holds one train per lane (64 pairs).  It is looked at only if it beats SOME lane's second best.  (Until
            // round 4 the tile's maximum was tested once and all 16 registers then went through the update -- with the trains
            // split into chunks for occupancy a wave sees few thousand of them, two thirds of its tiles held a new best-two for
            // one of its 64 queries, and the update sequence was half of the kernel's time: 252 M VALU instructions for
            // 40 000 x 40 000 descriptors.  Then one compare + scalar branch per register -- whose common case, "nothing
            // here", was a TAKEN branch, 16 per tile.)  Now two levels: the maximum of four registers (v_max3 + v_max)
            // against the second bests, falling through when nothing beats them; the four registers one by one only otherwise.
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int m = knn_max4(key[4 * g], key[4 * g + 1], key[4 * g + 2], key[4 * g + 3]);
                if (__builtin_expect(__ballot(m > bd1) == 0ull, 1)) continue;
#pragma unroll
                for (int r = 4 * g; r < 4 * g + 4; r++) {
                    const int d = key[r];
                    if (__ballot(d > bd1) == 0ull) continue;
                    const int ti = t0 + (r & 3) + 8 * (r >> 2);
                    if (d > bd0) { bd1 = bd0; bi1 = bi0; bd0 = d; bi0 = ti; }
                    else if (d > bd1) { bd1 = d; bi1 = ti; }
                }
            }
        }
        // (DB: no barrier here: the next step writes the OTHER copy, and this one is not written again before every wave has
        // passed the next barrier)
        if (!DB) __syncthreads();
    }
    // the two row-halves of a query (lanes l and l + 32) merge their best two; dot -> Hamming distance
    const int od0 = __shfl_xor(bd0, 32, 64), od1 = __shfl_xor(bd1, 32, 64);
    const int oi0 = __shfl_xor(bi0, 32, 64), oi1 = __shfl_xor(bi1, 32, 64);
    int d0 = bd0, d1 = bd1, i0 = bi0, i1 = bi1;
    const int cd[2] = { od0, od1 }; const int ci[2] = { oi0, oi1 };
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (ci[k] < 0) continue;
        if (i0 < 0 || knn_better(cd[k], ci[k], d0, i0)) { d1 = d0; i1 = i0; d0 = cd[k]; i0 = ci[k]; }
        else if (i1 < 0 || knn_better(cd[k], ci[k], d1, i1)) { d1 = cd[k]; i1 = ci[k]; }
    }
    const int q = q0 + li;
    if (lh == 0 && q < nq) {
        // key -> dot -> distance: dot = bits - 2 * distance (exact in either accumulator)
        auto dot_of = [](int key) -> int { return FP4 ? (int)(__builtin_bit_cast(float, key) - KNN_FP4_BIAS) : key; };
        Best2 b;
        b.d0 = i0 >= 0 ? (NBITS - dot_of(d0)) >> 1 : 0x7fffffff; b.i0 = i0;
        b.d1 = i1 >= 0 ? (NBITS - dot_of(d1)) >> 1 : 0x7fffffff; b.i1 = i1;
        partial[((size_t)blockIdx.z * J.nchunks + blockIdx.y) * J.cap + q] = b;
    }
}

// crossCheck: query i matches train j iff j is i's nearest train and i is j's nearest query
__global__ void crosscheck_kernel(const int* __restrict__ q2t, const int* __restrict__ t2q, int nq, int* __restrict__ match)
{
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const int j = q2t[2 * qi];
    match[qi] = (j >= 0 && t2q[2 * j] == qi) ? j : -1;
}

// ================================================================================================
// Mutual ratio-test matching on DEVICE row counts (efx_match_mutual_async / efx_match_mutual_batch_async): the
// filter of samples/sample_image_sequence.cpp:114-137 without a host round trip, on the knnMatch lists of both directions of
// every pair of a chain (jobs 2p and 2p + 1).  Pair = blockIdx.z.
// ================================================================================================

// the sample's three checks for query i of pair p (a ratio test passes when the second neighbour is missing: S15)
__device__ __forceinline__ bool mutual_keep(const KnnJobs& J, int p, int i, double ratio)
{
    const size_t a = 2 * ((size_t)(2 * p) * J.cap + i);
    const int j = J.idx[a];
    if (j < 0) return false;                               // no train row
    const size_t b = 2 * ((size_t)(2 * p + 1) * J.cap + j);
    return J.idx[b] == i && !(J.idx[a + 1] >= 0 && (double)J.dist[a] > ratio * (double)J.dist[a + 1])
                         && !(J.idx[b + 1] >= 0 && (double)J.dist[b] > ratio * (double)J.dist[b + 1]);
}

// kernel A of the ordered compaction: the accept flag of every query and the accepted count of every workgroup
__global__ __launch_bounds__(256) void mutual_flag_kernel(KnnJobs J, double ratio, uint8_t* __restrict__ flags, int* __restrict__ wgcount,
                                                          int nblk)
{
    __shared__ int s_n[4];
    const int p = blockIdx.z, tid = threadIdx.x;
    const int nq = knn_count(J.nq[p], J.q_cap);
    if ((int)blockIdx.x * 256 >= nq) return;
    const int i = blockIdx.x * 256 + tid;
    const bool ok = i < nq && mutual_keep(J, p, i, ratio);
    if (i < nq) flags[(size_t)p * J.q_cap + i] = ok ? 1 : 0;
    const unsigned long long m = __ballot(ok);
    if ((tid & 63) == 0) s_n[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) wgcount[(size_t)p * nblk + blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// kernel B: each workgroup sums the counts of the workgroups before it (in LDS; no communication between workgroups of this
// launch) and writes its accepted rows at their rank, in ascending query order; the last workgroup writes the total
__global__ __launch_bounds__(256) void mutual_compact_kernel(KnnJobs J, const uint8_t* __restrict__ flags, const int* __restrict__ wgcount,
                                                             int nblk)
{
    __shared__ int s_sum[4], s_n[4];
    const int p = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = knn_count(J.nq[p], J.q_cap);
    const int used = (nq + 255) >> 8, x = blockIdx.x;
    if (x >= used && x != 0) return;                       // (workgroup 0 writes the zero total of an empty query set)
    int s = 0;
    for (int k = tid; k < x; k += 256) s += wgcount[(size_t)p * nblk + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const int i = x * 256 + tid;
    const bool ok = i < nq && flags[(size_t)p * J.q_cap + i];
    const unsigned long long m = __ballot(ok);
    if (lane == 0) { s_sum[wave] = s; s_n[wave] = __popcll(m); }
    __syncthreads();
    const int base = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    int rank = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    for (int w = 0; w < wave; w++) rank += s_n[w];
    if (ok) {
        const size_t a = 2 * ((size_t)(2 * p) * J.cap + i);
        int* row = J.out[p] + 3 * (size_t)rank;
        row[0] = i; row[1] = J.idx[a]; row[2] = J.dist[a];
    }
    if (tid == 0 && x == (used > 0 ? used - 1 : 0)) *J.nout[p] = base + s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// the search kernel of a path (0: popcount on raw rows, 1: int8 matrix cores, 2: FP4 matrix cores, on expanded rows): the
// instantiation a launch runs and the occupancy query measures
const void* search_kernel(int path, int desc_bytes)
{
    const bool w256 = desc_bytes == 32;
    if (path == 0) return w256 ? reinterpret_cast<const void*>(&knn2_dc_kernel<8>) : reinterpret_cast<const void*>(&knn2_dc_kernel<16>);
    if (path == 1) return w256 ? reinterpret_cast<const void*>(&knn2_mfma_kernel<256, false>) : reinterpret_cast<const void*>(&knn2_mfma_kernel<512, false>);
    return w256 ? reinterpret_cast<const void*>(&knn2_mfma_kernel<256, true>) : reinterpret_cast<const void*>(&knn2_mfma_kernel<512, true>);
}

// the search of njobs jobs (grid: query blocks of J.cap x chunks x jobs), then the merge into their knnMatch lists
hipError_t knn_launch(KnnJobs J, int njobs, int path, int desc_bytes, void* partial, hipStream_t stream)
{
    if (J.nchunks < 1) return hipErrorInvalidValue;
    const unsigned xb = (unsigned)((J.cap + 255) / 256 > 0 ? (J.cap + 255) / 256 : 1);
    Best2* part = static_cast<Best2*>(partial);
    void* args[] = { &J, &part };
    hipError_t e = hipLaunchKernel(search_kernel(path, desc_bytes), dim3(xb, (unsigned)J.nchunks, (unsigned)njobs), dim3(path ? 512 : 256),
                                   args, 0, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn2_merge_dc_kernel, dim3(xb, 1, (unsigned)njobs), dim3(256), 0, stream, J, (const Best2*)part);
    return hipGetLastError();
}

// one job on host counts (knnMatch): NULL count pointers, i.e. counts = capacities
KnnJobs one_job(const uint8_t* q, size_t qp, int nq, const uint8_t* t, size_t tp, int nt, int nchunks, int* idx, int* dist)
{
    KnnJobs J = {};
    J.q[0] = q; J.t[0] = t; J.q_pitch = qp; J.t_pitch = tp;
    J.q_cap = nq; J.t_cap = nt; J.cap = nq; J.nchunks = nchunks;
    J.idx = idx; J.dist = dist;
    return J;
}

} // namespace

// matrix-core path: scratch_x holds the expanded queries and trains, efx_knn2_mfma_scratch() bytes (room for the int8 form)
size_t efx_knn2_mfma_scratch(int nq, int nt, int desc_bytes)
{
    return ((size_t)((nq + 255) & ~255) + (size_t)((nt + 255) & ~255)) * (size_t)desc_bytes * 8;
}

// Workgroups of the matrix-core kernel the chip holds at once (CUs x resident workgroups per CU, from the runtime's occupancy
// calculation for the instantiation that will launch): the host sizes the train chunks by it
int efx_knn2_mfma_resident_workgroups(int desc_bytes, int fp4)
{
    // per device (CU count and occupancy differ between devices), written by whichever thread asks first: atomics
    static std::atomic<int> cache[16][2][2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    std::atomic<int>* slot = (dev >= 0 && dev < 16) ? &cache[dev][desc_bytes == 32 ? 0 : 1][fp4 ? 1 : 0] : nullptr;
    if (slot) { const int c = slot->load(std::memory_order_relaxed); if (c > 0) return c; }
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, search_kernel(fp4 ? 2 : 1, desc_bytes), 512, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    if (slot) slot->store(per_cu * cus, std::memory_order_relaxed);
    return per_cu * cus;
}

// Expands nmat (<= 2 * EFX_MAX_BATCH) descriptor matrices in one launch: matrix i -> dst[i], room for round_up(cap[i], 256) rows of
// efx_mutual_expanded_row(desc_bytes, fp4) bytes; cap_max: the largest cap[i]
size_t efx_mutual_expanded_row(int desc_bytes, int fp4) { return (size_t)desc_bytes * (fp4 ? 4 : 8); }

hipError_t efx_launch_mutual_expand(int nmat, const uint8_t* const* src, const size_t* pitch, const int* const* n, const int* cap,
                                    int cap_max, int desc_bytes, int fp4, uint8_t* const* dst, hipStream_t stream)
{
    const size_t rows_pad = (size_t)((cap_max + 255) & ~255);
    if (nmat <= 0 || rows_pad == 0) return hipSuccess;
    if (nmat > 2 * EFX_MAX_BATCH) return hipErrorInvalidValue;
    ExpandJobs E = {};
    for (int i = 0; i < nmat; i++) { E.src[i] = src[i]; E.pitch[i] = pitch[i]; E.n[i] = n[i]; E.cap[i] = cap[i]; E.dst[i] = dst[i]; }
    const size_t g = rows_pad * (size_t)(desc_bytes / 2);
    const dim3 grid((unsigned)((g + 255) / 256), 1, (unsigned)nmat);
    if (fp4) hipLaunchKernelGGL(expand_dc_kernel<true>, grid, dim3(256), 0, stream, E, desc_bytes);
    else hipLaunchKernelGGL(expand_dc_kernel<false>, grid, dim3(256), 0, stream, E, desc_bytes);
    return hipGetLastError();
}

// knnMatch on the matrix cores: query and train expanded in one launch, then one job
hipError_t efx_launch_knn2_mfma(const uint8_t* query, size_t q_pitch, int nq, const uint8_t* train, size_t t_pitch, int nt,
                                int desc_bytes, void* scratch_x, void* scratch, int nchunks, int* idx, int* dist, hipStream_t stream, int fp4)
{
    if (nq <= 0) return hipSuccess;
    const size_t xrow = efx_mutual_expanded_row(desc_bytes, fp4);
    uint8_t* xq = static_cast<uint8_t*>(scratch_x);
    uint8_t* xt = xq + (size_t)((nq + 255) & ~255) * xrow;
    const uint8_t* src[2] = { query, train };
    const size_t pitch[2] = { q_pitch, t_pitch };
    const int* n[2] = { nullptr, nullptr };
    const int cap[2] = { nq, nt };
    uint8_t* const dst[2] = { xq, xt };
    const hipError_t e = efx_launch_mutual_expand(2, src, pitch, n, cap, nq > nt ? nq : nt, desc_bytes, fp4, dst, stream);
    if (e != hipSuccess) return e;
    return knn_launch(one_job(xq, xrow, nq, xt, xrow, nt, nchunks, idx, dist), 1, fp4 ? 2 : 1, desc_bytes, scratch, stream);
}

hipError_t efx_launch_knn2(const uint8_t* query, size_t q_pitch, int nq, const uint8_t* train, size_t t_pitch, int nt,
                           int desc_bytes, void* scratch, int nchunks, int* idx, int* dist, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    return knn_launch(one_job(query, q_pitch, nq, train, t_pitch, nt, nchunks, idx, dist), 1, 0, desc_bytes, scratch, stream);
}

hipError_t efx_launch_crosscheck(const int* q2t, const int* t2q, int nq, int* match, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(crosscheck_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, q2t, t2q, nq, match);
    return hipGetLastError();
}

// ---- mutual matching on device counts (efx_api.cpp: efx_match_mutual_async / efx_match_mutual_batch_async) ----
// One chain of npairs (<= EFX_MAX_BATCH) pairs: search both directions (one launch), merge (one), flag (one), compact (one).
// path 0: popcount on the raw rows q / t; 1: int8 matrix cores, 2: FP4 matrix cores, on expanded rows.  Scratch (bytes):
// partial 2 npairs x nchunks x cap x 16, knn 2 npairs x cap x 16 (knnMatch lists: idx, then dist), flags npairs x q_cap,
// wgcount npairs x ceil(q_cap / 256) x 4, cap = max(q_cap, t_cap)
hipError_t efx_launch_mutual(int npairs, const uint8_t* const* q, const uint8_t* const* t, const int* const* nq, const int* const* nt,
                             size_t q_pitch, size_t t_pitch, int q_cap, int t_cap, int desc_bytes, double ratio,
                             int* const* out, int* const* nout, int path, int nchunks,
                             void* partial, void* knn, void* flags, void* wgcount, hipStream_t stream)
{
    if (npairs <= 0) return hipSuccess;
    if (npairs > EFX_MAX_BATCH) return hipErrorInvalidValue;
    KnnJobs J = {};
    for (int p = 0; p < npairs; p++) { J.q[p] = q[p]; J.t[p] = t[p]; J.nq[p] = nq[p]; J.nt[p] = nt[p]; J.out[p] = out[p]; J.nout[p] = nout[p]; }
    J.q_pitch = q_pitch; J.t_pitch = t_pitch;
    J.q_cap = q_cap; J.t_cap = t_cap; J.cap = q_cap > t_cap ? q_cap : t_cap;
    J.nchunks = nchunks;
    J.idx = static_cast<int*>(knn);
    J.dist = J.idx + (size_t)(2 * npairs) * 2 * J.cap;
    hipError_t e = knn_launch(J, 2 * npairs, path, desc_bytes, partial, stream);
    if (e != hipSuccess) return e;
    const int nblk = (q_cap + 255) / 256 > 0 ? (q_cap + 255) / 256 : 1;
    const dim3 fgrid((unsigned)nblk, 1, (unsigned)npairs);
    hipLaunchKernelGGL(mutual_flag_kernel, fgrid, dim3(256), 0, stream, J, ratio, static_cast<uint8_t*>(flags), static_cast<int*>(wgcount), nblk);
    hipLaunchKernelGGL(mutual_compact_kernel, fgrid, dim3(256), 0, stream, J, (const uint8_t*)flags, (const int*)wgcount, nblk);
    return hipGetLastError();
}

// The flag + compact half of the chain above on knnMatch lists another search wrote (guided matching, guided_kernels.hip): knn
// holds idx, then dist, 2 npairs x cap x 2 ints each, jobs 2 p (query -> train) and 2 p + 1 (train -> query) of pair p
hipError_t efx_launch_mutual_filter(int npairs, const int* const* nq, int q_cap, int cap, double ratio, int* const* out, int* const* nout,
                                    void* knn, void* flags, void* wgcount, hipStream_t stream)
{
    if (npairs <= 0) return hipSuccess;
    if (npairs > EFX_MAX_BATCH) return hipErrorInvalidValue;
    KnnJobs J = {};
    for (int p = 0; p < npairs; p++) { J.nq[p] = nq[p]; J.out[p] = out[p]; J.nout[p] = nout[p]; }
    J.q_cap = q_cap; J.cap = cap;
    J.idx = static_cast<int*>(knn);
    J.dist = J.idx + (size_t)(2 * npairs) * 2 * J.cap;
    const int nblk = (q_cap + 255) / 256 > 0 ? (q_cap + 255) / 256 : 1;
    const dim3 fgrid((unsigned)nblk, 1, (unsigned)npairs);
    hipLaunchKernelGGL(mutual_flag_kernel, fgrid, dim3(256), 0, stream, J, ratio, static_cast<uint8_t*>(flags), static_cast<int*>(wgcount), nblk);
    hipLaunchKernelGGL(mutual_compact_kernel, fgrid, dim3(256), 0, stream, J, (const uint8_t*)flags, (const int*)wgcount, nblk);
    return hipGetLastError();
}
