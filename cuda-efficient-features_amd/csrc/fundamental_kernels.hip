// fundamental_kernels.hip -- RANSAC fundamental-matrix verification of matched keypoints on the device.
// One model per (query, train) pair with x'^T F x ~ 0 (x query, x' train).  The launch structure is that of the homography chain
// (homography_kernels.hip, section 5d): up to EFX_MAX_BATCH pairs per chain (pair = blockIdx.z), seven launches (five without the
// refit), no communication between the workgroups of one launch:
//   hom_gather_kernel  (ransac_common.h) match rows + LOCATION rows -> one float4 {x, y, x', y'} per row
//   fun_hyp_kernel     one lane per hypothesis: eight-draw sampler, exact location check, the 7 x 8 system relative to sample
//                      point 0 eliminated with complete pivoting in one LDS column per lane -> 9 fp32 coefficients
//   fun_score_kernel   the hot path: hypothesis blocks x match chunks x pairs; a lane owns two matches on packed fp32 math
//   fun_mask_kernel    row chunks x pairs: the winner (argmax), the mask, per-workgroup integer centroid sums
//   fun_dist_kernel    row chunks x pairs (refit only): per-workgroup sums of the distances to the centroids
//   fun_normal_kernel  row chunks x pairs (refit only): per-workgroup sums of the 36 distinct entries of A^T A
//   fun_finish_kernel  one workgroup per pair: the partial sums in workgroup order, two cyclic Jacobi solves (9 x 9, 3 x 3), the
//                      rank-2 model and the efx_fundamental record
// Row counts are read on the device; grids are sized from capacities and the hypothesis budget; parameters travel by value.

#include "ransac_common.h"             // job table, gather kernel, splitmix64, fixed-order sums, argmax, Hartley pass

namespace {

#define FUN_HB 32            // hypotheses per score workgroup
#define FUN_ROWS 512         // matches per score workgroup: 256 lanes x 2
#define FUN_COEF 16          // floats per hypothesis record: 9 coefficients, the valid flag, padding
#define FUN_NSUM 36          // distinct sums of A^T A (S18 step 7): {UU UV VV U V 1} x {uu uv vv u v 1}
#define FUN_HT 64            // threads of a hypothesis workgroup: one LDS column of 64 doubles per lane (32 KB per workgroup)
#define FUN_SWEEPS9 8        // cyclic Jacobi sweeps of the 9 x 9 solve, fixed (converged to rounding after 6 on every fit tried)
#define FUN_SWEEPS3 6        // and of the 3 x 3 solve

typedef RansacJobs FunJobs;

struct F9 { double v[9]; };

// ---- S18 steps 2-4: sampler, location check, eight-point model.  A: 64 doubles of LDS owned by this lane, entry k at A[k * st]
// (the 7 x 8 matrix row-major in 0..55, the unknowns in 56..63): data-dependent row and column swaps index LDS, never registers.
__device__ bool fun_model(const float4* __restrict__ P, int n, uint64_t seed, int h, double* A, int st, F9& F)
{
    if (n < 8) return false;
    // eight distinct indices: each draw skips the indices taken before it, in ascending order (srt: the earlier draws, sorted)
    uint32_t idx[8], srt[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t r = splitmix64(seed + 8ull * (uint64_t)h + (uint64_t)j);
        uint32_t v = (uint32_t)(((r >> 32) * (uint64_t)(n - j)) >> 32);
#pragma unroll
        for (int k = 0; k < j; k++)
            if (v >= srt[k]) v++;
        idx[j] = v;
        srt[j] = v;
#pragma unroll
        for (int k = j; k > 0; k--) {
            const uint32_t lo = min(srt[k - 1], srt[k]), hi = max(srt[k - 1], srt[k]);
            srt[k - 1] = lo; srt[k] = hi;
        }
    }
    int x[8], y[8], u[8], w[8];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float4 q = P[idx[k]];
        ok = ok && q.x == q.x;                                 // a row with an out-of-range index is NaN
        x[k] = (int)q.x; y[k] = (int)q.y; u[k] = (int)q.z; w[k] = (int)q.w;
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
#pragma unroll
        for (int j = i + 1; j < 8; j++)
            ok = ok && !(x[i] == x[j] && y[i] == y[j]) && !(u[i] == u[j] && w[i] == w[j]);
    }
    if (!ok) return false;
    // rows [u x, u y, u, v x, v y, v, x, y] of points 1..7 relative to point 0: exact integers below 2^34
#pragma unroll
    for (int k = 1; k < 8; k++) {
        const long long dx = x[k] - x[0], dy = y[k] - y[0], du = u[k] - u[0], dv = w[k] - w[0];
        double* r = A + (k - 1) * 8 * st;
        r[0] = (double)(du * dx); r[st] = (double)(du * dy); r[2 * st] = (double)du; r[3 * st] = (double)(dv * dx);
        r[4 * st] = (double)(dv * dy); r[5 * st] = (double)dv; r[6 * st] = (double)dx; r[7 * st] = (double)dy;
    }
    uint32_t perm = 0x76543210u;                               // column c holds unknown (perm >> 4 c) & 15
    // every loop is unrolled: the LDS reads of a pivot search or an elimination step are then issued together, not one per round trip
#pragma unroll
    for (int c = 0; c < 7; c++) {
        double best = -1.0;
        int pr = c, pc = c;
#pragma unroll
        for (int r = c; r < 7; r++)
#pragma unroll
            for (int j = c; j < 8; j++) {
                const double a = fabs(A[(r * 8 + j) * st]);
                if (a > best) { best = a; pr = r; pc = j; }
            }
        if (!(best > 0.0)) { ok = false; break; }
        if (pr != c)
#pragma unroll
            for (int j = 0; j < 8; j++) { const double s = A[(c * 8 + j) * st]; A[(c * 8 + j) * st] = A[(pr * 8 + j) * st]; A[(pr * 8 + j) * st] = s; }
        if (pc != c) {
#pragma unroll
            for (int r = 0; r < 7; r++) { const double s = A[(r * 8 + c) * st]; A[(r * 8 + c) * st] = A[(r * 8 + pc) * st]; A[(r * 8 + pc) * st] = s; }
            const uint32_t a = (perm >> (4 * c)) & 15u, b = (perm >> (4 * pc)) & 15u;
            perm = (perm & ~((15u << (4 * c)) | (15u << (4 * pc)))) | (b << (4 * c)) | (a << (4 * pc));
        }
        const double d = A[(c * 8 + c) * st];
#pragma unroll
        for (int r = c + 1; r < 7; r++) {
            const double f = A[(r * 8 + c) * st] / d;
#pragma unroll
            for (int j = c; j < 8; j++) A[(r * 8 + j) * st] = A[(r * 8 + j) * st] - f * A[(c * 8 + j) * st];
        }
    }
    if (!ok) return false;
    // back substitution, the free unknown = 1
    double* Z = A + 56 * st;
    Z[7 * st] = 1.0;
#pragma unroll
    for (int r = 6; r >= 0; r--) {
        double s = 0.0;
#pragma unroll
        for (int j = r + 1; j < 8; j++) s = s + A[(r * 8 + j) * st] * Z[j * st];
        Z[r * st] = (0.0 - s) / A[(r * 8 + r) * st];
    }
    // undo the column permutation through entries 0..7 (the matrix is no longer needed)
#pragma unroll
    for (int j = 0; j < 8; j++) A[((perm >> (4 * j)) & 15u) * st] = Z[j * st];
    const double f0 = A[0], f1 = A[st], f2 = A[2 * st], f3 = A[3 * st], f4 = A[4 * st], f5 = A[5 * st], f6 = A[6 * st], f7 = A[7 * st];
    // F = T'^T F_t T, T = [[1 0 -ox] [0 1 -oy] [0 0 1]], T' likewise with (ou, ov); F_t[8] = 0
    const double ox = (double)x[0], oy = (double)y[0], ou = (double)u[0], ov = (double)w[0];
    const double g2 = f2 - (f0 * ox + f1 * oy);
    const double g5 = f5 - (f3 * ox + f4 * oy);
    const double g8 = 0.0 - (f6 * ox + f7 * oy);
    const double r6 = f6 - (ou * f0 + ov * f3);
    const double r7 = f7 - (ou * f1 + ov * f4);
    const double r8 = g8 - (ou * g2 + ov * g5);
    F.v[0] = f0; F.v[1] = f1; F.v[2] = g2; F.v[3] = f3; F.v[4] = f4; F.v[5] = g5; F.v[6] = r6; F.v[7] = r7; F.v[8] = r8;
    double m = 0.0, d = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (fabs(F.v[k]) > m) { m = fabs(F.v[k]); d = F.v[k]; }
    if (d == 0.0) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        F.v[k] = F.v[k] / d;
        ok = ok && __builtin_isfinite(F.v[k]);
    }
    return ok;
}

// ---- S18 step 5: the Sampson test, fp32, in exactly this order (no contraction: -ffp-contract=off) ----
__device__ __forceinline__ bool fun_inlier(const float* f, float t2, float4 q)
{
    const float x = q.x, y = q.y, u = q.z, v = q.w;
    const float a = (f[0] * x + f[1] * y) + f[2];
    const float b = (f[3] * x + f[4] * y) + f[5];
    const float c = (f[6] * x + f[7] * y) + f[8];
    const float a2 = (f[0] * u + f[3] * v) + f[6];
    const float b2 = (f[1] * u + f[4] * v) + f[7];
    const float r = (a * u + b * v) + c;
    const float g = (a * a + b * b) + (a2 * a2 + b2 * b2);
    return g > 0.f && r * r <= t2 * g;
}

// ---- kernel 2: one lane per hypothesis; the count starts at 0 (valid) or -1 (invalid) ----
__global__ __launch_bounds__(FUN_HT) void fun_hyp_kernel(FunJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                         float* __restrict__ coef, int* __restrict__ cnt)
{
    __shared__ double s_A[64 * FUN_HT];
    const int p = blockIdx.z, h = blockIdx.x * FUN_HT + threadIdx.x;
    if (h >= J.hyps) return;
    F9 F;
    const bool ok = fun_model(pts + (size_t)p * J.cap, nrow[p], J.seed, h, s_A + threadIdx.x, FUN_HT, F);
    float4* c = reinterpret_cast<float4*>(coef + ((size_t)p * J.hyps + h) * FUN_COEF);
    if (ok) {
        c[0] = make_float4((float)F.v[0], (float)F.v[1], (float)F.v[2], (float)F.v[3]);
        c[1] = make_float4((float)F.v[4], (float)F.v[5], (float)F.v[6], (float)F.v[7]);
        c[2] = make_float4((float)F.v[8], 1.f, 0.f, 0.f);
    } else {
        c[0] = c[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        c[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    cnt[(size_t)p * J.hyps + h] = ok ? 0 : -1;
}

// ---- kernel 3: score.  Workgroup (x, y, p): hypotheses x * FUN_HB .. + FUN_HB of pair p against its rows y * 512 .. + 512.
// A lane owns rows r and r + 256 as one float2 pair (v_pk_mul_f32 / v_pk_add_f32); the coefficients are wave-uniform scalar
// loads.  Per hypothesis: two ballots and popcounts per wave into LDS, then one atomicAdd per hypothesis per workgroup.
typedef float f2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void fun_score_kernel(FunJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                        const float* __restrict__ coef, int* __restrict__ cnt)
{
    __shared__ int s_cnt[4][FUN_HB];
    const int p = blockIdx.z, tid = threadIdx.x, wave = tid >> 6;
    const int n = nrow[p];
    const int base = blockIdx.y * FUN_ROWS;
    if (base >= n) return;
    const int h0 = blockIdx.x * FUN_HB;
    const int hn = min(FUN_HB, J.hyps - h0);
    const float4* P = pts + (size_t)p * J.cap;
    const float4 nanv = make_float4(hom_nan(), hom_nan(), hom_nan(), hom_nan());
    const int r0 = base + tid, r1 = r0 + 256;
    const float4 qa = r0 < n ? P[r0] : nanv, qb = r1 < n ? P[r1] : nanv;
    const f2 x = { qa.x, qb.x }, y = { qa.y, qb.y }, u = { qa.z, qb.z }, v = { qa.w, qb.w };
    const float t2 = J.thr * J.thr;
    const float* C = coef + ((size_t)p * J.hyps + h0) * FUN_COEF;
    // the records are read one hypothesis ahead: the next record's scalar loads are in flight while this one is scored
    const float4* rec = reinterpret_cast<const float4*>(C);
    float4 n0 = rec[0], n1 = rec[1], n2 = rec[2];
    for (int i = 0; i < hn; i++) {
        const float4 c0 = n0, c1 = n1, c2 = n2;
        const float4* nx = reinterpret_cast<const float4*>(C + min(i + 1, hn - 1) * FUN_COEF);
        n0 = nx[0]; n1 = nx[1]; n2 = nx[2];
        int s = 0;
        if (c2.y != 0.f) {
            const f2 a = (c0.x * x + c0.y * y) + c0.z;
            const f2 b = (c0.w * x + c1.x * y) + c1.y;
            const f2 c = (c1.z * x + c1.w * y) + c2.x;
            const f2 a2 = (c0.x * u + c0.w * v) + c1.z;
            const f2 b2 = (c0.y * u + c1.x * v) + c1.w;
            const f2 r = (a * u + b * v) + c;
            const f2 g = (a * a + b * b) + (a2 * a2 + b2 * b2);
            const f2 l = r * r, m = t2 * g;
            const unsigned long long m0 = __ballot(g.x > 0.f && l.x <= m.x);
            const unsigned long long m1 = __ballot(g.y > 0.f && l.y <= m.y);
            s = __popcll(m0) + __popcll(m1);
        }
        s_cnt[wave][i] = s;                        // every lane writes the wave's value
    }
    __syncthreads();
    if (tid < hn) {
        const int s = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        if (s > 0) atomicAdd(&cnt[(size_t)p * J.hyps + h0 + tid], s);
    }
}

// pass 1, grid ceil(capacity / 256) x 1 x pairs: the winner (workgroup 0 records it: best, index, valid count), the mask of the
// workgroup's rows (0 past the count and without a model), the integer coordinate sums of its inliers
__global__ __launch_bounds__(HOM_RB) void fun_mask_kernel(FunJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                          const float* __restrict__ coef, const int* __restrict__ cnt,
                                                          int* __restrict__ sel, long long* __restrict__ pa, int nblk)
{
    __shared__ int s_i[12];
    __shared__ long long s_ll[4];
    const int p = blockIdx.z, tid = threadIdx.x, k = blockIdx.x * HOM_RB + tid;
    const int n = nrow[p];
    int best, bi, nv;
    hom_argmax(cnt + (size_t)p * J.hyps, J.hyps, best, bi, nv, s_i);
    if (blockIdx.x == 0 && tid == 0) { sel[4 * p] = best; sel[4 * p + 1] = bi; sel[4 * p + 2] = nv; }
    bool in = false;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (best >= 0 && k < n) {
        q = pts[(size_t)p * J.cap + k];
        in = fun_inlier(coef + ((size_t)p * J.hyps + bi) * FUN_COEF, J.thr * J.thr, q);
    }
    if (k < J.cap) J.mask[p][k] = in ? 1 : 0;
    const long long v0 = block_sum_ll(in ? (long long)q.x : 0, s_ll), v1 = block_sum_ll(in ? (long long)q.y : 0, s_ll);
    const long long v2 = block_sum_ll(in ? (long long)q.z : 0, s_ll), v3 = block_sum_ll(in ? (long long)q.w : 0, s_ll);
    if (tid == 0) {
        long long* o = pa + ((size_t)p * nblk + blockIdx.x) * 4;
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
    }
}

__device__ __forceinline__ bool fun_refits(const FunJobs& J, const int* sel, int p) { return J.refine && sel[4 * p] >= 8; }

// pass 2 (refit only): the distances of the workgroup's inliers to the centroids, query and train side
__global__ __launch_bounds__(HOM_RB) void fun_dist_kernel(FunJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                          const float* __restrict__ coef, const int* __restrict__ sel,
                                                          const long long* __restrict__ pa, double* __restrict__ pb, int nblk)
{
    __shared__ long long s_ll[4];
    __shared__ double s_red[2][HOM_RB / 64];
    const int p = blockIdx.z, tid = threadIdx.x, k = blockIdx.x * HOM_RB + tid;
    if (!fun_refits(J, sel, p)) return;
    const int n = nrow[p], best = sel[4 * p], bi = sel[4 * p + 1];
    double c[4];
    hom_centroids(pa, p, nblk, (double)best, c, s_ll);
    double d[2] = { 0.0, 0.0 };
    if (k < n) {
        const float4 q = pts[(size_t)p * J.cap + k];
        if (fun_inlier(coef + ((size_t)p * J.hyps + bi) * FUN_COEF, J.thr * J.thr, q)) {
            const double ax = (double)q.x - c[0], ay = (double)q.y - c[1], bx = (double)q.z - c[2], by = (double)q.w - c[3];
            d[0] = sqrt(ax * ax + ay * ay);
            d[1] = sqrt(bx * bx + by * by);
        }
    }
    block_sum<2>(d, s_red);
    if (tid == 0) { double* o = pb + ((size_t)p * nblk + blockIdx.x) * 2; o[0] = d[0]; o[1] = d[1]; }
}

// pass 3 (refit only): the 36 distinct sums of A^T A over the workgroup's normalised inliers, sum 6 a + b = train monomial a
// times query monomial b of {UU UV VV U V 1} x {uu uv vv u v 1}
__global__ __launch_bounds__(HOM_RB) void fun_normal_kernel(FunJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                            const float* __restrict__ coef, const int* __restrict__ sel,
                                                            const long long* __restrict__ pa, const double* __restrict__ pb,
                                                            double* __restrict__ pc, int nblk)
{
    __shared__ long long s_ll[4];
    __shared__ double s_red[FUN_NSUM][HOM_RB / 64];
    const int p = blockIdx.z, tid = threadIdx.x, k = blockIdx.x * HOM_RB + tid;
    if (!fun_refits(J, sel, p)) return;
    const int n = nrow[p], best = sel[4 * p], bi = sel[4 * p + 1];
    double c[4], ss, sd;
    hom_hartley(pa, pb, p, nblk, best, c, ss, sd, s_ll, s_red);
    double S[FUN_NSUM];
#pragma unroll
    for (int i = 0; i < FUN_NSUM; i++) S[i] = 0.0;
    if (k < n) {
        const float4 q = pts[(size_t)p * J.cap + k];
        if (fun_inlier(coef + ((size_t)p * J.hyps + bi) * FUN_COEF, J.thr * J.thr, q)) {
            const double u = ss * ((double)q.x - c[0]), v = ss * ((double)q.y - c[1]);
            const double U = sd * ((double)q.z - c[2]), V = sd * ((double)q.w - c[3]);
            const double tm[6] = { U * U, U * V, V * V, U, V, 1.0 };
            const double qm[6] = { u * u, u * v, v * v, u, v, 1.0 };
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int b = 0; b < 6; b++) S[6 * a + b] = tm[a] * qm[b];
            }
        }
    }
    block_sum<FUN_NSUM>(S, s_red);
    if (tid == 0) {
        double* o = pc + ((size_t)p * nblk + blockIdx.x) * FUN_NSUM;
#pragma unroll
        for (int i = 0; i < FUN_NSUM; i++) o[i] = S[i];
    }
}

// index of the product of two of {U, V, 1} (or {u, v, 1}) in {UU UV VV U V 1}
__device__ __forceinline__ int fun_mono(int a, int b)
{
    const int lo = min(a, b), hi = max(a, b);
    return hi == 2 ? 3 + lo : lo + hi;
}

// Cyclic Jacobi on the symmetric n x n matrix in M[0] (LDS, row-major, n <= 9), by the whole workgroup: `sweeps` sweeps of n rounds;
// round r rotates the disjoint index pairs {i, (r - i) mod n} at once (every pair once per sweep), M <- J^T M J, V <- V J.  The
// rotation of (p, q), p < q, with a = Mqq - Mpp and b = 2 Mpq: h = sqrt(a a + b b), t = b / (a + sign(a) h), c = 1 / sqrt(t t + 1),
// s = t c; Mpq == 0: none.  cs[i] / cs[9 + i]: column i becomes cs[i] * column i + cs[9 + i] * column partner(i).  M and V are
// double-buffered (two barriers per round); returns the buffer that holds the result.
__device__ int fun_jacobi(int n, int sweeps, double (*M)[81], double (*V)[81], double* cs)
{
    const int tid = threadIdx.x, i = tid / n, j = tid % n;
    const bool act = tid < n * n;
    if (act) V[0][i * n + j] = i == j ? 1.0 : 0.0;
    int cur = 0;
    __syncthreads();
    for (int sweep = 0; sweep < sweeps; sweep++) {
        for (int r = 0; r < n; r++) {
            const double* Mc = M[cur];
            const double* Vc = V[cur];
            if (tid < n) {
                const int q = (r - tid + n) % n;
                if (q == tid) { cs[tid] = 1.0; cs[9 + tid] = 0.0; }
                else if (tid < q) {
                    const double apq = Mc[tid * n + q];
                    double c = 1.0, s = 0.0;
                    if (apq != 0.0) {
                        const double a = Mc[q * n + q] - Mc[tid * n + tid], b = 2.0 * apq;
                        const double h = sqrt(a * a + b * b);
                        const double t = b / (a + (a >= 0.0 ? h : 0.0 - h));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                    }
                    cs[tid] = c; cs[9 + tid] = 0.0 - s;
                    cs[q] = c; cs[9 + q] = s;
                }
            }
            __syncthreads();
            if (act) {
                const int pj = (r - j + n) % n, pi = (r - i + n) % n;
                const double cj = cs[j], gj = cs[9 + j], ci = cs[i], gi = cs[9 + i];
                const double top = cj * Mc[i * n + j] + gj * Mc[i * n + pj];        // (M J)[i][j]
                const double bot = cj * Mc[pi * n + j] + gj * Mc[pi * n + pj];      // (M J)[partner(i)][j]
                M[cur ^ 1][i * n + j] = ci * top + gi * bot;
                V[cur ^ 1][i * n + j] = cj * Vc[i * n + j] + gj * Vc[i * n + pj];
            }
            cur ^= 1;
            __syncthreads();
        }
    }
    return cur;
}

// the index of the first smallest diagonal entry
__device__ __forceinline__ int fun_smallest(int n, const double* M)
{
    int k = 0;
    for (int i = 1; i < n; i++)
        if (M[i * n + i] < M[k * n + k]) k = i;
    return k;
}

// finish, one workgroup per pair: the record; with a refit A^T A from the partials, its smallest eigenvector, the rank-2
// projection and the denormalisation
__global__ __launch_bounds__(HOM_RB) void fun_finish_kernel(FunJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                            const int* __restrict__ sel, const long long* __restrict__ pa,
                                                            const double* __restrict__ pb, const double* __restrict__ pc, int nblk)
{
    __shared__ long long s_ll[4];
    __shared__ double s_red[FUN_NSUM][HOM_RB / 64];
    __shared__ double s_S[FUN_NSUM];
    __shared__ double s_M[2][81], s_V[2][81], s_cs[18], s_F[9], s_A[64];
    const int p = blockIdx.z, tid = threadIdx.x;
    const int n = nrow[p], best = sel[4 * p], bi = sel[4 * p + 1], nv = sel[4 * p + 2];
    efx_fundamental* R = static_cast<efx_fundamental*>(J.res[p]);
    if (best < 0) {                                // S18 step 8: no model (the mask pass wrote the zero mask)
        if (tid == 0) {
            for (int k = 0; k < 9; k++) R->F[k] = 0.0;
            R->ninliers = 0; R->hypothesis = -1; R->valid_hypotheses = 0; R->refined = 0;
        }
        return;
    }
    bool refined = false;
    double Fr[9];
    if (J.refine && best >= 8) {
        double c[4], ss, sd;
        hom_hartley(pa, pb, p, nblk, best, c, ss, sd, s_ll, s_red);
        double S[FUN_NSUM];
        partial_sum<FUN_NSUM>(pc, p, nblk, S, s_red);
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < FUN_NSUM; i++) s_S[i] = S[i];
        }
        __syncthreads();
        // A^T A of the rows [U u, U v, U, V u, V v, V, u, v, 1]: entry (i, j) = train monomial (i / 3, j / 3) x query monomial (i % 3, j % 3)
        if (tid < 81) {
            const int i = tid / 9, j = tid % 9;
            s_M[0][tid] = s_S[6 * fun_mono(i / 3, j / 3) + fun_mono(i % 3, j % 3)];
        }
        __syncthreads();
        const int b9 = fun_jacobi(9, FUN_SWEEPS9, s_M, s_V, s_cs);
        if (tid == 0) {
            const int k = fun_smallest(9, s_M[b9]);
            for (int i = 0; i < 9; i++) s_F[i] = s_V[b9][i * 9 + k];
        }
        __syncthreads();
        if (tid < 9) {                             // G = Fn^T Fn
            const int i = tid / 3, j = tid % 3;
            s_M[0][tid] = (s_F[i] * s_F[j] + s_F[3 + i] * s_F[3 + j]) + s_F[6 + i] * s_F[6 + j];
        }
        __syncthreads();
        const int b3 = fun_jacobi(3, FUN_SWEEPS3, s_M, s_V, s_cs);
        if (tid == 0) {
            const int k = fun_smallest(3, s_M[b3]);
            const double v0 = s_V[b3][k], v1 = s_V[b3][3 + k], v2 = s_V[b3][6 + k];
            double Fn[9];
#pragma unroll
            for (int i = 0; i < 3; i++) {          // Fn <- Fn - (Fn v3) v3^T
                const double w = (s_F[3 * i] * v0 + s_F[3 * i + 1] * v1) + s_F[3 * i + 2] * v2;
                Fn[3 * i] = s_F[3 * i] - w * v0; Fn[3 * i + 1] = s_F[3 * i + 1] - w * v1; Fn[3 * i + 2] = s_F[3 * i + 2] - w * v2;
            }
            // F = T_dst^T Fn T_src, T = [[s 0 -s cx] [0 s -s cy] [0 0 1]]
            double G[9];
#pragma unroll
            for (int i = 0; i < 3; i++) {          // Fn T_src
                G[3 * i] = Fn[3 * i] * ss; G[3 * i + 1] = Fn[3 * i + 1] * ss;
                G[3 * i + 2] = Fn[3 * i + 2] - (Fn[3 * i] * ss * c[0] + Fn[3 * i + 1] * ss * c[1]);
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Fr[j] = sd * G[j]; Fr[3 + j] = sd * G[3 + j];
                Fr[6 + j] = G[6 + j] - (sd * c[2] * G[j] + sd * c[3] * G[3 + j]);
            }
            double m = 0.0, d = 0.0;
#pragma unroll
            for (int k2 = 0; k2 < 9; k2++)
                if (fabs(Fr[k2]) > m) { m = fabs(Fr[k2]); d = Fr[k2]; }
            bool ok = d != 0.0;
#pragma unroll
            for (int k2 = 0; k2 < 9; k2++) { Fr[k2] = Fr[k2] / d; ok = ok && __builtin_isfinite(Fr[k2]); }
            refined = ok;
        }
    }
    if (tid == 0) {
        if (!refined) {
            F9 F;
            fun_model(pts + (size_t)p * J.cap, n, J.seed, bi, s_A, 1, F);   // the winner's eight-point model, recomputed bit for bit
#pragma unroll
            for (int k = 0; k < 9; k++) Fr[k] = F.v[k];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) R->F[k] = Fr[k];
        R->ninliers = best; R->hypothesis = bi; R->valid_hypotheses = nv; R->refined = refined ? 1 : 0;
    }
}

} // namespace

// Scratch of one chain of npairs pairs, capacity rows and hyps hypotheses (bytes): a 512-byte header (clamped counts, winners),
// gathered rows, hypothesis records, the row passes' partial sums (336 B per pass workgroup), counts.
size_t efx_fundamental_scratch(int npairs, int cap, int hyps)
{
    const size_t c = cap > 0 ? (size_t)cap : 1, nblk = (c + HOM_RB - 1) / HOM_RB;
    return 512 + (size_t)npairs * (c * 16 + (size_t)hyps * (FUN_COEF * 4 + 4) + nblk * (4 * 8 + 2 * 8 + FUN_NSUM * 8));
}

// One chain of npairs (<= EFX_MAX_BATCH) pairs: gather, hypotheses, score, the three row passes, finish.
hipError_t efx_launch_fundamental(int npairs, const void* const* kq, const void* const* kt, const int* const* m, const int* const* nm,
                                  int q_cap, int t_cap, int cap, int hyps, float thr, unsigned long long seed, int refine,
                                  efx_fundamental* const* res, uint8_t* const* mask, void* scratch, hipStream_t stream)
{
    if (npairs <= 0) return hipSuccess;
    if (npairs > EFX_MAX_BATCH || hyps < 1) return hipErrorInvalidValue;
    FunJobs J = {};
    for (int p = 0; p < npairs; p++) {
        J.kq[p] = static_cast<const uint32_t*>(kq[p]); J.kt[p] = static_cast<const uint32_t*>(kt[p]);
        J.m[p] = m[p]; J.nm[p] = nm ? nm[p] : nullptr; J.res[p] = res[p]; J.mask[p] = mask[p];
    }
    J.seed = seed; J.q_cap = q_cap; J.t_cap = t_cap; J.cap = cap; J.hyps = hyps; J.refine = refine; J.thr = thr;
    const size_t c = cap > 0 ? (size_t)cap : 1;
    const int nblk = (int)((c + HOM_RB - 1) / HOM_RB);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    int* nrow = reinterpret_cast<int*>(base);                           // EFX_MAX_BATCH ints
    int* sel = nrow + EFX_MAX_BATCH;                                     // 4 ints per pair
    float4* pts = reinterpret_cast<float4*>(base + 512);
    float* coef = reinterpret_cast<float*>(base + 512 + (size_t)npairs * c * 16);
    long long* pa = reinterpret_cast<long long*>(coef + (size_t)npairs * hyps * FUN_COEF);
    double* pb = reinterpret_cast<double*>(pa + (size_t)npairs * nblk * 4);
    double* pc = pb + (size_t)npairs * nblk * 2;
    int* cnt = reinterpret_cast<int*>(pc + (size_t)npairs * nblk * FUN_NSUM);
    const unsigned z = (unsigned)npairs;
    const unsigned gx = (unsigned)((c + 255) / 256), hx = (unsigned)((hyps + FUN_HT - 1) / FUN_HT);
    hipLaunchKernelGGL(hom_gather_kernel, dim3(gx, 1, z), dim3(256), 0, stream, J, pts, nrow);
    hipLaunchKernelGGL(fun_hyp_kernel, dim3(hx, 1, z), dim3(FUN_HT), 0, stream, J, (const float4*)pts, (const int*)nrow, coef, cnt);
    const unsigned sx = (unsigned)((hyps + FUN_HB - 1) / FUN_HB), sy = (unsigned)((c + FUN_ROWS - 1) / FUN_ROWS);
    hipLaunchKernelGGL(fun_score_kernel, dim3(sx, sy, z), dim3(256), 0, stream, J, (const float4*)pts, (const int*)nrow,
                       (const float*)coef, cnt);
    const dim3 rgrid((unsigned)nblk, 1, z);
    hipLaunchKernelGGL(fun_mask_kernel, rgrid, dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow, (const float*)coef,
                       (const int*)cnt, sel, pa, nblk);
    if (refine) {
        hipLaunchKernelGGL(fun_dist_kernel, rgrid, dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow,
                           (const float*)coef, (const int*)sel, (const long long*)pa, pb, nblk);
        hipLaunchKernelGGL(fun_normal_kernel, rgrid, dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow,
                           (const float*)coef, (const int*)sel, (const long long*)pa, (const double*)pb, pc, nblk);
    }
    hipLaunchKernelGGL(fun_finish_kernel, dim3(1, 1, z), dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow,
                       (const int*)sel, (const long long*)pa, (const double*)pb, (const double*)pc, nblk);
    return hipGetLastError();
}
