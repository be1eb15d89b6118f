// homography_kernels.hip -- RANSAC homography verification of matched keypoints on the device.
// One model per (query, train) pair maps query keypoints to train keypoints.  A launch chain serves up to EFX_MAX_BATCH pairs
// (pair = blockIdx.z) in seven launches (five without the refit), with no communication between the workgroups of one launch:
//   hom_gather_kernel  match rows + LOCATION rows -> one float4 {x, y, x', y'} per row (NaN for a row whose index is out of range)
//   hom_hyp_kernel     one lane per hypothesis: sampler, exact subset check, closed-form four-point model -> 9 fp32 coefficients
//   hom_score_kernel   the hot path: hypothesis blocks x match chunks x pairs; a lane owns two matches on packed fp32 math
//   hom_mask_kernel    row chunks x pairs: the winner (argmax), the mask, per-workgroup integer centroid sums
//   hom_dist_kernel    row chunks x pairs (refit only): per-workgroup sums of the distances to the centroids
//   hom_normal_kernel  row chunks x pairs (refit only): per-workgroup sums of the normal equations
//   hom_finish_kernel  one workgroup per pair: the partial sums in workgroup order, the 8 x 8 solve, the efx_homography record
// Row counts are read on the device (the gather kernel clamps them once); grids are sized from capacities and the hypothesis
// budget.  Parameters travel by value (HomJobs), so nothing host-written can be rewritten under queued work.

#include "ransac_common.h"             // job table, gather kernel, splitmix64, fixed-order sums, argmax, Hartley pass

namespace {

#define HOM_HB 32            // hypotheses per score workgroup
#define HOM_ROWS 512         // matches per score workgroup: 256 lanes x 2
#define HOM_COEF 16          // floats per hypothesis record: 9 coefficients, the valid flag, padding
#define HOM_NSUM 22          // distinct sums of the normal equations (S16 step 7)

typedef RansacJobs HomJobs;

// ---- S16 steps 2-4: sampler, subset check, closed-form four-point model ----

__device__ __forceinline__ uint32_t hom_draw(uint64_t seed, int h, int j, int n)
{
    const uint64_t r = splitmix64(seed + 4ull * (uint64_t)h + (uint64_t)j);
    return (uint32_t)(((r >> 32) * (uint64_t)(n - j)) >> 32);
}

__device__ __forceinline__ long long hom_cross(long long ax, long long ay, long long bx, long long by, long long cx, long long cy)
{
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

struct Quad { double a, b, c, d, e, f, g, h; };    // [[a b c] [d e f] [g h 1]]: unit square -> p0 p1 p2 p3

__device__ __forceinline__ Quad hom_quad(long long x0, long long y0, long long x1, long long y1, long long x2, long long y2,
                                         long long x3, long long y3)
{
    const long long sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
    const long long dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
    const long long den = dx1 * dy2 - dx2 * dy1;
    Quad q;
    q.g = (double)(sx * dy2 - dx2 * sy) / (double)den;
    q.h = (double)(dx1 * sy - sx * dy1) / (double)den;
    q.a = (double)(x1 - x0) + q.g * (double)x1;
    q.b = (double)(x3 - x0) + q.h * (double)x3;
    q.c = (double)x0;
    q.d = (double)(y1 - y0) + q.g * (double)y1;
    q.e = (double)(y3 - y0) + q.h * (double)y3;
    q.f = (double)y0;
    return q;
}

struct H9 { double v[9]; };

// Hypothesis h of a pair of n gathered rows: true and the model (H[8] == 1) when the sample is valid.
__device__ bool hom_model(const float4* __restrict__ P, int n, uint64_t seed, int h, H9& H)
{
    if (n < 4) return false;
    // four distinct indices: each draw skips the indices taken before it, in ascending order
    const uint32_t i0 = hom_draw(seed, h, 0, n);
    uint32_t v = hom_draw(seed, h, 1, n);
    if (v >= i0) v++;
    const uint32_t i1 = v;
    uint32_t s0 = min(i0, i1), s1 = max(i0, i1);
    v = hom_draw(seed, h, 2, n);
    if (v >= s0) v++;
    if (v >= s1) v++;
    const uint32_t i2 = v;
    const uint32_t t0 = min(s0, i2), t2 = max(s1, i2), t1 = max(s0, min(s1, i2));
    v = hom_draw(seed, h, 3, n);
    if (v >= t0) v++;
    if (v >= t1) v++;
    if (v >= t2) v++;
    const uint32_t i3 = v;
    const float4 a = P[i0], b = P[i1], c = P[i2], d = P[i3];
    if (a.x != a.x || b.x != b.x || c.x != c.x || d.x != d.x) return false;      // a row with an out-of-range index
    const long long x0 = (long long)a.x, y0 = (long long)a.y, u0 = (long long)a.z, w0 = (long long)a.w;
    const long long x1 = (long long)b.x, y1 = (long long)b.y, u1 = (long long)b.z, w1 = (long long)b.w;
    const long long x2 = (long long)c.x, y2 = (long long)c.y, u2 = (long long)c.z, w2 = (long long)c.w;
    const long long x3 = (long long)d.x, y3 = (long long)d.y, u3 = (long long)d.z, w3 = (long long)d.w;
    const long long s012 = hom_cross(x0, y0, x1, y1, x2, y2), d012 = hom_cross(u0, w0, u1, w1, u2, w2);
    const long long s013 = hom_cross(x0, y0, x1, y1, x3, y3), d013 = hom_cross(u0, w0, u1, w1, u3, w3);
    const long long s023 = hom_cross(x0, y0, x2, y2, x3, y3), d023 = hom_cross(u0, w0, u2, w2, u3, w3);
    const long long s123 = hom_cross(x1, y1, x2, y2, x3, y3), d123 = hom_cross(u1, w1, u2, w2, u3, w3);
    if (!s012 || !d012 || !s013 || !d013 || !s023 || !d023 || !s123 || !d123) return false;
    const int flips = ((s012 > 0) != (d012 > 0)) + ((s013 > 0) != (d013 > 0)) + ((s023 > 0) != (d023 > 0)) + ((s123 > 0) != (d123 > 0));
    if (flips != 0 && flips != 4) return false;
    const Quad S = hom_quad(x0, y0, x1, y1, x2, y2, x3, y3);
    const Quad D = hom_quad(u0, w0, u1, w1, u2, w2, u3, w3);
    // adj(Q_src), Q_src[2][2] = 1
    const double A00 = S.e - S.f * S.h, A01 = S.c * S.h - S.b, A02 = S.b * S.f - S.c * S.e;
    const double A10 = S.f * S.g - S.d, A11 = S.a - S.c * S.g, A12 = S.c * S.d - S.a * S.f;
    const double A20 = S.d * S.h - S.e * S.g, A21 = S.b * S.g - S.a * S.h, A22 = S.a * S.e - S.b * S.d;
    H.v[0] = (D.a * A00 + D.b * A10) + D.c * A20;
    H.v[1] = (D.a * A01 + D.b * A11) + D.c * A21;
    H.v[2] = (D.a * A02 + D.b * A12) + D.c * A22;
    H.v[3] = (D.d * A00 + D.e * A10) + D.f * A20;
    H.v[4] = (D.d * A01 + D.e * A11) + D.f * A21;
    H.v[5] = (D.d * A02 + D.e * A12) + D.f * A22;
    H.v[6] = (D.g * A00 + D.h * A10) + 1.0 * A20;
    H.v[7] = (D.g * A01 + D.h * A11) + 1.0 * A21;
    H.v[8] = (D.g * A02 + D.h * A12) + 1.0 * A22;
    const double h22 = H.v[8];
    if (h22 == 0.0) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        H.v[k] = H.v[k] / h22;
        ok = ok && __builtin_isfinite(H.v[k]);
    }
    return ok;
}

// ---- S16 step 5: the inlier test, fp32, in exactly this order (no contraction: -ffp-contract=off) ----
__device__ __forceinline__ bool hom_inlier(const float* c, float t2, float4 q)
{
    const float X = (c[0] * q.x + c[1] * q.y) + c[2];
    const float Y = (c[3] * q.x + c[4] * q.y) + c[5];
    const float W = (c[6] * q.x + c[7] * q.y) + c[8];
    const float ex = X - q.z * W, ey = Y - q.w * W;
    return W != 0.f && ex * ex + ey * ey <= t2 * (W * W);
}

// ---- kernel 2: one lane per hypothesis; the count starts at 0 (valid) or -1 (invalid) ----
__global__ __launch_bounds__(256) void hom_hyp_kernel(HomJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                      float* __restrict__ coef, int* __restrict__ cnt)
{
    const int p = blockIdx.z, h = blockIdx.x * 256 + threadIdx.x;
    if (h >= J.hyps) return;
    H9 H;
    const bool ok = hom_model(pts + (size_t)p * J.cap, nrow[p], J.seed, h, H);
    float4* c = reinterpret_cast<float4*>(coef + ((size_t)p * J.hyps + h) * HOM_COEF);
    if (ok) {
        c[0] = make_float4((float)H.v[0], (float)H.v[1], (float)H.v[2], (float)H.v[3]);
        c[1] = make_float4((float)H.v[4], (float)H.v[5], (float)H.v[6], (float)H.v[7]);
        c[2] = make_float4((float)H.v[8], 1.f, 0.f, 0.f);
    } else {
        c[0] = c[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        c[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    cnt[(size_t)p * J.hyps + h] = ok ? 0 : -1;
}

// ---- kernel 3: score.  Workgroup (x, y, p): hypotheses x * HOM_HB .. + HOM_HB of pair p against its rows y * 512 .. + 512.
// A lane owns rows r and r + 256 as one float2 pair (v_pk_mul_f32 / v_pk_add_f32); the coefficients are wave-uniform scalar
// loads.  Per hypothesis: two ballots and popcounts per wave into LDS, then one atomicAdd per hypothesis per workgroup.
typedef float f2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void hom_score_kernel(HomJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                        const float* __restrict__ coef, int* __restrict__ cnt)
{
    __shared__ int s_cnt[4][HOM_HB];
    const int p = blockIdx.z, tid = threadIdx.x, wave = tid >> 6;
    const int n = nrow[p];
    const int base = blockIdx.y * HOM_ROWS;
    if (base >= n) return;
    const int h0 = blockIdx.x * HOM_HB;
    const int hn = min(HOM_HB, J.hyps - h0);
    const float4* P = pts + (size_t)p * J.cap;
    const float4 nanv = make_float4(hom_nan(), hom_nan(), hom_nan(), hom_nan());
    const int r0 = base + tid, r1 = r0 + 256;
    const float4 a = r0 < n ? P[r0] : nanv, b = r1 < n ? P[r1] : nanv;
    const f2 x = { a.x, b.x }, y = { a.y, b.y }, xd = { a.z, b.z }, yd = { a.w, b.w };
    const float t2 = J.thr * J.thr;
    const float* C = coef + ((size_t)p * J.hyps + h0) * HOM_COEF;
    // the records are read one hypothesis ahead: the next record's scalar loads are in flight while this one is scored
    const float4* rec = reinterpret_cast<const float4*>(C);
    float4 n0 = rec[0], n1 = rec[1], n2 = rec[2];
    for (int i = 0; i < hn; i++) {
        const float4 c0 = n0, c1 = n1, c2 = n2;
        const float4* nx = reinterpret_cast<const float4*>(C + min(i + 1, hn - 1) * HOM_COEF);
        n0 = nx[0]; n1 = nx[1]; n2 = nx[2];
        int s = 0;
        if (c2.y != 0.f) {
            const f2 X = (c0.x * x + c0.y * y) + c0.z;
            const f2 Y = (c0.w * x + c1.x * y) + c1.y;
            const f2 W = (c1.z * x + c1.w * y) + c2.x;
            const f2 ex = X - xd * W, ey = Y - yd * W;
            const f2 l = ex * ex + ey * ey, r = t2 * (W * W);
            const unsigned long long m0 = __ballot(W.x != 0.f && l.x <= r.x);
            const unsigned long long m1 = __ballot(W.y != 0.f && l.y <= r.y);
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
__global__ __launch_bounds__(HOM_RB) void hom_mask_kernel(HomJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
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
        in = hom_inlier(coef + ((size_t)p * J.hyps + bi) * HOM_COEF, J.thr * J.thr, q);
    }
    if (k < J.cap) J.mask[p][k] = in ? 1 : 0;
    const long long v0 = block_sum_ll(in ? (long long)q.x : 0, s_ll), v1 = block_sum_ll(in ? (long long)q.y : 0, s_ll);
    const long long v2 = block_sum_ll(in ? (long long)q.z : 0, s_ll), v3 = block_sum_ll(in ? (long long)q.w : 0, s_ll);
    if (tid == 0) {
        long long* o = pa + ((size_t)p * nblk + blockIdx.x) * 4;
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
    }
}

__device__ __forceinline__ bool hom_refits(const HomJobs& J, const int* sel, int p) { return J.refine && sel[4 * p] >= 4; }

// pass 2 (refit only): the distances of the workgroup's inliers to the centroids, src and dst
__global__ __launch_bounds__(HOM_RB) void hom_dist_kernel(HomJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                          const float* __restrict__ coef, const int* __restrict__ sel,
                                                          const long long* __restrict__ pa, double* __restrict__ pb, int nblk)
{
    __shared__ long long s_ll[4];
    __shared__ double s_red[2][HOM_RB / 64];
    const int p = blockIdx.z, tid = threadIdx.x, k = blockIdx.x * HOM_RB + tid;
    if (!hom_refits(J, sel, p)) return;
    const int n = nrow[p], best = sel[4 * p], bi = sel[4 * p + 1];
    double c[4];
    hom_centroids(pa, p, nblk, (double)best, c, s_ll);
    double d[2] = { 0.0, 0.0 };
    if (k < n) {
        const float4 q = pts[(size_t)p * J.cap + k];
        if (hom_inlier(coef + ((size_t)p * J.hyps + bi) * HOM_COEF, J.thr * J.thr, q)) {
            const double ax = (double)q.x - c[0], ay = (double)q.y - c[1], bx = (double)q.z - c[2], by = (double)q.w - c[3];
            d[0] = sqrt(ax * ax + ay * ay);
            d[1] = sqrt(bx * bx + by * by);
        }
    }
    block_sum<2>(d, s_red);
    if (tid == 0) { double* o = pb + ((size_t)p * nblk + blockIdx.x) * 2; o[0] = d[0]; o[1] = d[1]; }
}

// pass 3 (refit only): the 22 distinct sums of the normal equations over the workgroup's normalised inliers
__global__ __launch_bounds__(HOM_RB) void hom_normal_kernel(HomJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                            const float* __restrict__ coef, const int* __restrict__ sel,
                                                            const long long* __restrict__ pa, const double* __restrict__ pb,
                                                            double* __restrict__ pc, int nblk)
{
    __shared__ long long s_ll[4];
    __shared__ double s_red[HOM_NSUM][HOM_RB / 64];
    const int p = blockIdx.z, tid = threadIdx.x, k = blockIdx.x * HOM_RB + tid;
    if (!hom_refits(J, sel, p)) return;
    const int n = nrow[p], best = sel[4 * p], bi = sel[4 * p + 1];
    double c[4], ss, sd;
    hom_hartley(pa, pb, p, nblk, best, c, ss, sd, s_ll, s_red);
    double S[HOM_NSUM];
#pragma unroll
    for (int i = 0; i < HOM_NSUM; i++) S[i] = 0.0;
    if (k < n) {
        const float4 q = pts[(size_t)p * J.cap + k];
        if (hom_inlier(coef + ((size_t)p * J.hyps + bi) * HOM_COEF, J.thr * J.thr, q)) {
            const double u = ss * ((double)q.x - c[0]), v = ss * ((double)q.y - c[1]);
            const double U = sd * ((double)q.z - c[2]), V = sd * ((double)q.w - c[3]);
            const double uu = u * u, uv = u * v, vv = v * v, r = U * U + V * V;
            S[0] = uu; S[1] = uv; S[2] = vv; S[3] = u; S[4] = v;
            S[5] = U * uu; S[6] = U * uv; S[7] = U * vv; S[8] = U * u; S[9] = U * v;
            S[10] = V * uu; S[11] = V * uv; S[12] = V * vv; S[13] = V * u; S[14] = V * v;
            S[15] = r * uu; S[16] = r * uv; S[17] = r * vv; S[18] = U; S[19] = V; S[20] = r * u; S[21] = r * v;
        }
    }
    block_sum<HOM_NSUM>(S, s_red);
    if (tid == 0) {
        double* o = pc + ((size_t)p * nblk + blockIdx.x) * HOM_NSUM;
#pragma unroll
        for (int i = 0; i < HOM_NSUM; i++) o[i] = S[i];
    }
}

// finish, one workgroup per pair: the record; with a refit the normal equations from the partials, Gaussian elimination with
// partial pivoting on 72 threads, back substitution and denormalisation
__global__ __launch_bounds__(HOM_RB) void hom_finish_kernel(HomJobs J, const float4* __restrict__ pts, const int* __restrict__ nrow,
                                                            const int* __restrict__ sel, const long long* __restrict__ pa,
                                                            const double* __restrict__ pb, const double* __restrict__ pc, int nblk)
{
    __shared__ long long s_ll[4];
    __shared__ double s_red[HOM_NSUM][HOM_RB / 64];
    __shared__ double s_A[8][9];
    __shared__ double s_x[8];
    __shared__ int s_piv, s_fail;
    const int p = blockIdx.z, tid = threadIdx.x;
    const int n = nrow[p], best = sel[4 * p], bi = sel[4 * p + 1], nv = sel[4 * p + 2];
    efx_homography* R = static_cast<efx_homography*>(J.res[p]);
    if (best < 0) {                                // S16 step 8: no model (the mask pass wrote the zero mask)
        if (tid == 0) {
            for (int k = 0; k < 9; k++) R->H[k] = 0.0;
            R->ninliers = 0; R->hypothesis = -1; R->valid_hypotheses = 0; R->refined = 0;
        }
        return;
    }
    bool refined = false;
    double Hr[9];
    if (J.refine && best >= 4) {
        double c[4], ss, sd;
        hom_hartley(pa, pb, p, nblk, best, c, ss, sd, s_ll, s_red);
        double S[HOM_NSUM];
        partial_sum<HOM_NSUM>(pc, p, nblk, S, s_red);
        if (tid == 0) {
            // A^T A | A^T b of the h22 = 1 DLT rows [u v 1 0 0 0 -uU -vU | U] and [0 0 0 u v 1 -uV -vV | V]
            const double N = (double)best;
            const double row[8][9] = {
                { S[0], S[1], S[3], 0, 0, 0, -S[5], -S[6], S[8] },
                { S[1], S[2], S[4], 0, 0, 0, -S[6], -S[7], S[9] },
                { S[3], S[4], N, 0, 0, 0, -S[8], -S[9], S[18] },
                { 0, 0, 0, S[0], S[1], S[3], -S[10], -S[11], S[13] },
                { 0, 0, 0, S[1], S[2], S[4], -S[11], -S[12], S[14] },
                { 0, 0, 0, S[3], S[4], N, -S[13], -S[14], S[19] },
                { -S[5], -S[6], -S[8], -S[10], -S[11], -S[13], S[15], S[16], -S[20] },
                { -S[6], -S[7], -S[9], -S[11], -S[12], -S[14], S[16], S[17], -S[21] },
            };
#pragma unroll
            for (int i = 0; i < 8; i++) {
#pragma unroll
                for (int j = 0; j < 9; j++) s_A[i][j] = row[i][j];
            }
            s_fail = 0;
        }
        __syncthreads();
        // thread (r, j) = (tid / 9, tid % 9) owns one entry; each entry gets the serial algorithm's value: f = A[r][col] / A[col][col]
        // is read before any entry of the step changes
        const int er = tid / 9, ej = tid % 9;
        for (int col = 0; col < 8; col++) {
            if (tid == 0) {
                int piv = col;
                for (int r = col + 1; r < 8; r++)
                    if (fabs(s_A[r][col]) > fabs(s_A[piv][col])) piv = r;
                s_piv = piv;
                if (s_A[piv][col] == 0.0) s_fail = 1;
            }
            __syncthreads();
            if (s_fail) break;
            const int piv = s_piv;
            if (piv != col && tid < 9) { const double t = s_A[col][tid]; s_A[col][tid] = s_A[piv][tid]; s_A[piv][tid] = t; }
            __syncthreads();
            double nvv = 0.0;
            const bool upd = tid < 72 && er > col && ej >= col;
            if (upd) {
                const double f = s_A[er][col] / s_A[col][col];
                nvv = s_A[er][ej] - f * s_A[col][ej];
            }
            __syncthreads();
            if (upd) s_A[er][ej] = nvv;
            __syncthreads();
        }
        if (tid == 0) {
            bool ok = !s_fail;
            if (ok) {
                for (int r = 7; r >= 0; r--) {
                    double s = s_A[r][8];
                    for (int j = r + 1; j < 8; j++) s -= s_A[r][j] * s_x[j];
                    s_x[r] = s / s_A[r][r];
                }
                // H = T_dst^-1 Hn T_src, T = [[s 0 -s cx] [0 s -s cy] [0 0 1]]
                const double n0 = s_x[0], n1 = s_x[1], n2 = s_x[2], n3 = s_x[3], n4 = s_x[4], n5 = s_x[5], n6 = s_x[6], n7 = s_x[7];
                const double cxs = c[0], cys = c[1], cxd = c[2], cyd = c[3];
                const double m0 = n0 * ss, m1 = n1 * ss, m2 = n2 - (n0 * ss * cxs + n1 * ss * cys);          // Hn T_src
                const double m3 = n3 * ss, m4 = n4 * ss, m5 = n5 - (n3 * ss * cxs + n4 * ss * cys);
                const double m6 = n6 * ss, m7 = n7 * ss, m8 = 1.0 - (n6 * ss * cxs + n7 * ss * cys);
                const double id = 1.0 / sd;
                Hr[0] = id * m0 + cxd * m6; Hr[1] = id * m1 + cxd * m7; Hr[2] = id * m2 + cxd * m8;
                Hr[3] = id * m3 + cyd * m6; Hr[4] = id * m4 + cyd * m7; Hr[5] = id * m5 + cyd * m8;
                Hr[6] = m6; Hr[7] = m7; Hr[8] = m8;
                const double h22 = Hr[8];
                ok = h22 != 0.0;
                for (int k = 0; k < 9; k++) { Hr[k] = Hr[k] / h22; ok = ok && __builtin_isfinite(Hr[k]); }
            }
            refined = ok;
        }
    }
    if (tid == 0) {
        if (!refined) {
            H9 H;
            hom_model(pts + (size_t)p * J.cap, n, J.seed, bi, H);   // the winner's four-point model, recomputed bit for bit
            for (int k = 0; k < 9; k++) Hr[k] = H.v[k];
        }
        for (int k = 0; k < 9; k++) R->H[k] = Hr[k];
        R->ninliers = best; R->hypothesis = bi; R->valid_hypotheses = nv; R->refined = refined ? 1 : 0;
    }
}

} // namespace

// Scratch of one chain of npairs pairs, capacity rows and hyps hypotheses (bytes): a 512-byte header (clamped counts, winners),
// gathered rows, hypothesis records, the row passes' partial sums (224 B per pass workgroup), counts.
size_t efx_homography_scratch(int npairs, int cap, int hyps)
{
    const size_t c = cap > 0 ? (size_t)cap : 1, nblk = (c + HOM_RB - 1) / HOM_RB;
    return 512 + (size_t)npairs * (c * 16 + (size_t)hyps * (HOM_COEF * 4 + 4) + nblk * (4 * 8 + 2 * 8 + HOM_NSUM * 8));
}

// One chain of npairs (<= EFX_MAX_BATCH) pairs: gather, hypotheses, score, the three row passes, finish.
hipError_t efx_launch_homography(int npairs, const void* const* kq, const void* const* kt, const int* const* m, const int* const* nm,
                                 int q_cap, int t_cap, int cap, int hyps, float thr, unsigned long long seed, int refine,
                                 efx_homography* const* res, uint8_t* const* mask, void* scratch, hipStream_t stream)
{
    if (npairs <= 0) return hipSuccess;
    if (npairs > EFX_MAX_BATCH || hyps < 1) return hipErrorInvalidValue;
    HomJobs J = {};
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
    long long* pa = reinterpret_cast<long long*>(coef + (size_t)npairs * hyps * HOM_COEF);
    double* pb = reinterpret_cast<double*>(pa + (size_t)npairs * nblk * 4);
    double* pc = pb + (size_t)npairs * nblk * 2;
    int* cnt = reinterpret_cast<int*>(pc + (size_t)npairs * nblk * HOM_NSUM);
    const unsigned z = (unsigned)npairs;
    const unsigned gx = (unsigned)((c + 255) / 256), hx = (unsigned)((hyps + 255) / 256);
    hipLaunchKernelGGL(hom_gather_kernel, dim3(gx, 1, z), dim3(256), 0, stream, J, pts, nrow);
    hipLaunchKernelGGL(hom_hyp_kernel, dim3(hx, 1, z), dim3(256), 0, stream, J, (const float4*)pts, (const int*)nrow, coef, cnt);
    const unsigned sx = (unsigned)((hyps + HOM_HB - 1) / HOM_HB), sy = (unsigned)((c + HOM_ROWS - 1) / HOM_ROWS);
    hipLaunchKernelGGL(hom_score_kernel, dim3(sx, sy, z), dim3(256), 0, stream, J, (const float4*)pts, (const int*)nrow,
                       (const float*)coef, cnt);
    const dim3 rgrid((unsigned)nblk, 1, z);
    hipLaunchKernelGGL(hom_mask_kernel, rgrid, dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow, (const float*)coef,
                       (const int*)cnt, sel, pa, nblk);
    if (refine) {
        hipLaunchKernelGGL(hom_dist_kernel, rgrid, dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow,
                           (const float*)coef, (const int*)sel, (const long long*)pa, pb, nblk);
        hipLaunchKernelGGL(hom_normal_kernel, rgrid, dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow,
                           (const float*)coef, (const int*)sel, (const long long*)pa, (const double*)pb, pc, nblk);
    }
    hipLaunchKernelGGL(hom_finish_kernel, dim3(1, 1, z), dim3(HOM_RB), 0, stream, J, (const float4*)pts, (const int*)nrow,
                       (const int*)sel, (const long long*)pa, (const double*)pb, (const double*)pc, nblk);
    return hipGetLastError();
}
