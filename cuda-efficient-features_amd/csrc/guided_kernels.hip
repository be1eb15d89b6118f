// guided_kernels.hip -- guided (spatially gated) mutual matching on the device (efx_match_guided_async /
// efx_match_guided_batch_async): the mutual ratio-test filter of S15 with both knnMatch directions
// restricted to the candidate pairs C = { (i, j) : train j lies in the square window of `radius` around the position a prior
// homography predicts for query i (and their octaves are close enough) }.
//
// A chain serves up to EFX_MAX_BATCH pairs.  Every distinct (descriptor matrix, keypoint matrix, count, prior) of a chain is one BIN
// (at most 2 * EFX_MAX_BATCH): its rows are sorted by the cell of a uniform grid their predicted position falls into (a train
// matrix, or a query matrix without a prior: its own location), by a counting sort in four launches --
//   guided_bin_kernel      one lane per row: prediction (double, S17 step 2), cell, integer atomicAdd histogram (the value the atomic
//                          returns is the row's rank inside its cell, so the scatter needs no second atomic)
//   guided_cellsum_kernel, guided_scan_kernel   exclusive scan of the cell counts in two grid passes with per-workgroup partial sums
//   guided_scatter_kernel  one lane per row: original index, octave, prediction and the descriptor row into cell order
// -- and one search launch over both directions of every pair (job z = 2 p + direction, as the brute-force family):
//   guided_search_kernel   eight lanes per row; they share the candidates of the (at most) 3 x 3 cells around the row's position,
//                          walked as one list, apply the EXACT gate of S17 step 3, XOR + popcount the survivors and reduce the best two on the packed
//                          key (distance << 32 | original index) with three xor-shuffles.  It writes knnMatch lists in the layout
//                          of the brute-force path, so mutual_flag_kernel / mutual_compact_kernel (match_kernels.hip) finish the job.
// The order of rows inside a cell is whatever the atomics give; it cannot reach the output (the key holds the original index).
// Rows whose prediction does not exist (W <= 0, not finite, a prior without a model) go to an extra cell behind the grid that no
// walk visits: they get empty lists.  Cell coordinates are clamped to the grid; clamping is monotone, so the clamped cell range of
// [position - radius - 1, position + radius + 1] holds every row that can pass the gate, wherever positions lie (the one pixel of
// slack covers the rounding of the doubles involved; beyond 2^21 pixels nothing passes a window of at most 32 768 anyway, and a
// larger radius uses a grid of ONE cell).  No workgroup waits for another, no floating-point atomics, no private segment.

#include "efx_device.h"
#include "../../include/efx.h"

namespace {

#ifndef GUIDED_LANES
#define GUIDED_LANES 8                    // lanes per row in the search (4 / 8 / 16 measured: DESIGN.md section 5e)
#endif
#define GUIDED_INVALID_KEY 0xffffffffffffffffull

struct GuidedGrid {
    int x0, y0;                           // origin
    int edge;                             // cell edge in pixels, > radius
    int gw, gh;                           // cells; gw * gh = ncells, cell ncells holds the rows without a prediction
};

struct GuidedJobs {                       // a chain, passed by value
    const uint8_t* desc[2 * EFX_MAX_BATCH];       // per bin: descriptor rows, keypoint matrix, device count, prior (NULL: none)
    const uint8_t* kps[2 * EFX_MAX_BATCH];
    const int* cnt[2 * EFX_MAX_BATCH];
    const efx_homography* prior[2 * EFX_MAX_BATCH];
    size_t dpitch[2 * EFX_MAX_BATCH], kpitch[2 * EFX_MAX_BATCH];
    int cap[2 * EFX_MAX_BATCH];
    int qbin[EFX_MAX_BATCH], tbin[EFX_MAX_BATCH]; // per pair: the bins of its query and train side
    // scratch, one array per line of efx_guided_scratch(), bin b at b x the per-bin length: cell counts (ncells + 1), their sums
    // per scan workgroup, cell starts (ncells + 2); per row (`rows` = the largest capacity): cell, rank and prediction in original
    // order; original index, octave, prediction and descriptor in cell order
    int* count; int* wgsum; int* start; int* cell; int* rank; double2* pred;
    int* sidx; int* soct; double2* spred; uint8_t* sdesc;
    int rows;
    GuidedGrid g;
    float radius; int max_octave_diff;
    int desc_bytes;
    int* idx; int* dist; int cap_max;             // knnMatch lists of job z (the brute-force path's layout, row stride cap_max)
};

__device__ __forceinline__ int guided_count(const int* p, int cap)
{
    if (!p) return cap;
    const int n = *p;
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// cell coordinate of position v along one axis: floor((v - origin) / edge) clamped to [0, cells - 1]; monotone in v, and exact for
// integer v (the quotient of two integers below 2^18 is further from the next integer than a double's rounding)
__device__ __forceinline__ int guided_cell(double v, int origin, int edge, int cells)
{
    const double t = v - (double)origin;
    if (!(t > 0.0)) return 0;
    const double c = floor(t / (double)edge);
    return c >= (double)(cells - 1) ? cells - 1 : (int)c;
}

// S17 step 2 for row i of bin b: the predicted position, or false when there is none
__device__ __forceinline__ bool guided_predict(const GuidedJobs& G, int b, int i, double2* out)
{
    const int loc = reinterpret_cast<const int*>(G.kps[b])[i];
    const double x = (double)(short)(loc & 0xffff), y = (double)(short)(loc >> 16);
    const efx_homography* pr = G.prior[b];
    if (!pr) { *out = make_double2(x, y); return true; }
    if (pr->hypothesis < 0) { *out = make_double2(0.0, 0.0); return false; }
    const double* H = pr->H;
    const double X = (H[0] * x + H[1] * y) + H[2];
    const double Y = (H[3] * x + H[4] * y) + H[5];
    const double W = (H[6] * x + H[7] * y) + H[8];
    const double px = X / W, py = Y / W;
    *out = make_double2(px, py);
    return W > 0.0 && isfinite(px) && isfinite(py);
}

__global__ __launch_bounds__(256) void guided_bin_kernel(GuidedJobs G)
{
    const int b = blockIdx.z;
    const int n = guided_count(G.cnt[b], G.cap[b]);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ncells = G.g.gw * G.g.gh;
    double2 p;
    int c = ncells;
    if (guided_predict(G, b, i, &p))
        c = guided_cell(p.y, G.g.y0, G.g.edge, G.g.gh) * G.g.gw + guided_cell(p.x, G.g.x0, G.g.edge, G.g.gw);
    const size_t r = (size_t)b * G.rows + i;
    G.cell[r] = c;
    G.rank[r] = atomicAdd(&G.count[(size_t)b * (ncells + 1) + c], 1);
    G.pred[r] = p;
}

// The exclusive scan of a bin's cell counts in two grid passes (the structure of mutual_flag_kernel / mutual_compact_kernel):
// every workgroup owns GUIDED_SCAN_CELLS consecutive counts (four per thread).  Pass one: their sum.
#define GUIDED_SCAN_CELLS 1024
__global__ __launch_bounds__(256) void guided_cellsum_kernel(GuidedJobs G, int nblk)
{
    __shared__ int s_n[4];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int nc = G.g.gw * G.g.gh + 1;                    // counts
    const int* cnt = G.count + (size_t)b * nc;
    const int c0 = blockIdx.x * GUIDED_SCAN_CELLS + 4 * tid;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) if (c0 + k < nc) s += cnt[c0 + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) s_n[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) G.wgsum[(size_t)b * nblk + blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// Pass two: start[c] = rows in cells before c, c = 0 .. ncells + 1 (start[ncells]: the rows with a prediction, start[ncells + 1]:
// all rows).  A workgroup adds up the sums of the workgroups before it (no communication between workgroups of this launch) and
// scans its own counts behind that
__global__ __launch_bounds__(256) void guided_scan_kernel(GuidedJobs G, int nblk)
{
    __shared__ int s_sum[4], s_n[4];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc = G.g.gw * G.g.gh + 1;
    const int* cnt = G.count + (size_t)b * nc;
    int* st = G.start + (size_t)b * (nc + 1);
    int before = 0;
    for (int k = tid; k < (int)blockIdx.x; k += 256) before += G.wgsum[(size_t)b * nblk + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    const int c0 = blockIdx.x * GUIDED_SCAN_CELLS + 4 * tid;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = c0 + k < nc ? cnt[c0 + k] : 0; s += v[k]; }
    int inc = s;                                           // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    if (lane == 0) s_sum[wave] = before;
    if (lane == 63) s_n[wave] = inc;
    __syncthreads();
    int base = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3] + inc - s;
    for (int w = 0; w < wave; w++) base += s_n[w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (c0 + k < nc) st[c0 + k] = base;
        base += v[k];
        if (c0 + k == nc - 1) st[nc] = base;               // behind the last count: every row
    }
}

__global__ __launch_bounds__(256) void guided_scatter_kernel(GuidedJobs G)
{
    const int b = blockIdx.z;
    const int n = guided_count(G.cnt[b], G.cap[b]);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ncells = G.g.gw * G.g.gh;
    const size_t r = (size_t)b * G.rows + i;
    const int c = G.cell[r];
    const size_t pos = (size_t)b * G.rows + (size_t)(G.start[(size_t)b * (ncells + 2) + c] + G.rank[r]);
    G.sidx[pos] = i;
    G.soct[pos] = G.max_octave_diff >= 0 ? reinterpret_cast<const int*>(G.kps[b] + 3 * G.kpitch[b])[i] : 0;
    G.spred[pos] = G.pred[r];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(G.desc[b] + (size_t)i * G.dpitch[b]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(G.sdesc + pos * (size_t)G.desc_bytes);
    const int nw = G.desc_bytes >> 2;
    for (int k = 0; k < nw; k++) dst[k] = src[k];
}

// the two smallest keys of (a0 <= a1) and (b0 <= b1)
__device__ __forceinline__ void guided_merge(unsigned long long& a0, unsigned long long& a1, unsigned long long b0, unsigned long long b1)
{
    const unsigned long long lo = a0 < b0 ? a0 : b0, hi = a0 < b0 ? b0 : a0;
    const unsigned long long m = a1 < b1 ? a1 : b1;
    a0 = lo; a1 = hi < m ? hi : m;
}

// Job z = 2 p + direction: direction 0 gives every query of pair p its best two trains inside C, direction 1 every train its
// best two queries inside C.  A group of GUIDED_LANES lanes serves the row at one position of its own bin's cell order (neighbours
// in a wave are neighbours in the frame: their candidates are the same cache lines).
template <int NW>   // dwords per descriptor
__global__ __launch_bounds__(256) void guided_search_kernel(GuidedJobs G)
{
    constexpr int GPB = 256 / GUIDED_LANES;                // rows per workgroup
    const int z = blockIdx.z, p = z >> 1, dir = z & 1;
    const int A = dir ? G.tbin[p] : G.qbin[p], B = dir ? G.qbin[p] : G.tbin[p];
    const int n = guided_count(G.cnt[A], G.cap[A]);
    if ((int)blockIdx.x * GPB >= n) return;
    const int sub = threadIdx.x & (GUIDED_LANES - 1);
    const int r = blockIdx.x * GPB + (threadIdx.x / GUIDED_LANES);
    const bool live = r < n;
    const int ncells = G.g.gw * G.g.gh;
    const int* stA = G.start + (size_t)A * (ncells + 2);
    const int* stB = G.start + (size_t)B * (ncells + 2);
    const size_t ra = (size_t)A * G.rows + (live ? r : 0), rb = (size_t)B * G.rows;
    unsigned long long k0 = GUIDED_INVALID_KEY, k1 = GUIDED_INVALID_KEY;
    if (live && r < stA[ncells]) {                         // the row has a position
        const double2 P = G.spred[ra];
        const int oct = G.soct[ra];
        uint32_t q[NW];
        {
            const uint4* qp = reinterpret_cast<const uint4*>(G.sdesc + ra * (size_t)(4 * NW));
#pragma unroll
            for (int k = 0; k < NW / 4; k++) { const uint4 v = qp[k]; q[4 * k] = v.x; q[4 * k + 1] = v.y; q[4 * k + 2] = v.z; q[4 * k + 3] = v.w; }
        }
        const double R = (double)G.radius, reach = R + 1.0;
        const int xlo = guided_cell(P.x - reach, G.g.x0, G.g.edge, G.g.gw), xhi = guided_cell(P.x + reach, G.g.x0, G.g.edge, G.g.gw);
        const int ylo = guided_cell(P.y - reach, G.g.y0, G.g.edge, G.g.gh), yhi = guided_cell(P.y + reach, G.g.y0, G.g.edge, G.g.gh);
        // The cells xlo .. xhi of a grid row are one contiguous run of the cell order.  A window spans at most three grid rows:
        // their runs are walked as ONE list, so a row's few candidates are independent loads spread over its lanes
        for (int cy = ylo; cy <= yhi; cy += 3) {
            const bool h1 = cy + 1 <= yhi, h2 = cy + 2 <= yhi;
            const int s0 = stB[cy * G.g.gw + xlo], n0 = stB[cy * G.g.gw + xhi + 1] - s0;
            const int s1 = h1 ? stB[(cy + 1) * G.g.gw + xlo] : 0, n1 = h1 ? stB[(cy + 1) * G.g.gw + xhi + 1] - s1 : 0;
            const int s2 = h2 ? stB[(cy + 2) * G.g.gw + xlo] : 0, n2 = h2 ? stB[(cy + 2) * G.g.gw + xhi + 1] - s2 : 0;
            for (int t = sub; t < n0 + n1 + n2; t += GUIDED_LANES) {
                const int k = t < n0 ? s0 + t : (t < n0 + n1 ? s1 + (t - n0) : s2 + (t - n0 - n1));
                const double2 Q = G.spred[rb + k];
                // the gate of S17 step 3, fabs(train position - predicted query position): in direction 1 this row is the train
                const double dx = dir ? P.x - Q.x : Q.x - P.x, dy = dir ? P.y - Q.y : Q.y - P.y;
                if (!(fabs(dx) <= R && fabs(dy) <= R)) continue;
                if (G.max_octave_diff >= 0) {
                    const int d = (int)((unsigned)oct - (unsigned)G.soct[rb + k]);
                    if (!((d < 0 ? (int)(0u - (unsigned)d) : d) <= G.max_octave_diff)) continue;
                }
                const uint4* tp = reinterpret_cast<const uint4*>(G.sdesc + (rb + k) * (size_t)(4 * NW));
                int dist = 0;
#pragma unroll
                for (int w = 0; w < NW / 4; w++) {
                    const uint4 v = tp[w];
                    dist += __popc(q[4 * w] ^ v.x) + __popc(q[4 * w + 1] ^ v.y) + __popc(q[4 * w + 2] ^ v.z) + __popc(q[4 * w + 3] ^ v.w);
                }
                const unsigned long long key = ((unsigned long long)(unsigned)dist << 32) | (unsigned)G.sidx[rb + k];
                if (key < k0) { k1 = k0; k0 = key; } else if (key < k1) k1 = key;
            }
        }
    }
#pragma unroll
    for (int o = 1; o < GUIDED_LANES; o <<= 1) {
        const unsigned long long o0 = __shfl_xor(k0, o, 64), o1 = __shfl_xor(k1, o, 64);
        guided_merge(k0, k1, o0, o1);
    }
    if (live && sub == 0) {
        const size_t w = 2 * ((size_t)z * G.cap_max + G.sidx[ra]);
        const bool h0 = k0 != GUIDED_INVALID_KEY, h1 = k1 != GUIDED_INVALID_KEY;
        G.idx[w] = h0 ? (int)(unsigned)k0 : -1; G.idx[w + 1] = h1 ? (int)(unsigned)k1 : -1;
        G.dist[w] = h0 ? (int)(k0 >> 32) : -1; G.dist[w + 1] = h1 ? (int)(k1 >> 32) : -1;
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

} // namespace

// The grid of a call, from its parameters alone (never from device data).  The cell edge exceeds the radius by a pixel (three
// cells then cover the reach of radius + 1 on either side of a position) and is at least 16; it doubles until the grid has at
// most 2^18 cells.  width / height only size the grid: positions outside it fall into its border cells.
void efx_guided_grid(float radius, int width, int height, int* x0, int* y0, int* edge, int* gw, int* gh)
{
    if (!(radius <= 32768.f)) { *x0 = *y0 = -32768; *edge = 1 << 17; *gw = *gh = 1; return; }
    long e = (long)ceilf(radius) + 1;
    if (e < 16) e = 16;
    const long xr = width > 0 ? width : 65536, yr = height > 0 ? height : 65536;
    while (((xr + e - 1) / e) * ((yr + e - 1) / e) > (1L << 18)) e *= 2;
    *x0 = width > 0 ? 0 : -32768; *y0 = height > 0 ? 0 : -32768;
    *edge = (int)e; *gw = (int)((xr + e - 1) / e); *gh = (int)((yr + e - 1) / e);
}

// scratch of a chain of nbins bins of up to `rows` rows on a grid of ncells cells: the counts of every bin first (one memset)
size_t efx_guided_scratch(int nbins, int rows, int ncells, int desc_bytes)
{
    const size_t b = (size_t)nbins, r = (size_t)(rows > 0 ? rows : 1);
    return align256(b * (ncells + 1) * 4) + align256(b * ((ncells + 1 + GUIDED_SCAN_CELLS - 1) / GUIDED_SCAN_CELLS) * 4) + align256(b * (ncells + 2) * 4) + 4 * align256(b * r * 4) + 2 * align256(b * r * 16) +
           align256(b * r * (size_t)desc_bytes);
}

// One chain: nbins (<= 2 * EFX_MAX_BATCH) bins, npairs (<= EFX_MAX_BATCH) pairs whose sides are bins qbin[p] / tbin[p].  Writes
// the knnMatch lists of jobs 2 p, 2 p + 1 into knn (idx, then dist: 2 npairs x cap_max x 2 ints each), cap_max = the largest capacity.
hipError_t efx_launch_guided_search(int nbins, const uint8_t* const* desc, const size_t* dpitch, const uint8_t* const* kps,
                                    const size_t* kpitch, const int* const* cnt, const int* cap, const efx_homography* const* prior,
                                    int npairs, const int* qbin, const int* tbin, int cap_max, int desc_bytes,
                                    float radius, int max_octave_diff, int width, int height,
                                    void* scratch, void* knn, hipStream_t stream)
{
    if (npairs <= 0 || nbins <= 0) return hipSuccess;
    if (npairs > EFX_MAX_BATCH || nbins > 2 * EFX_MAX_BATCH) return hipErrorInvalidValue;
    GuidedJobs G = {};
    for (int b = 0; b < nbins; b++) {
        G.desc[b] = desc[b]; G.dpitch[b] = dpitch[b]; G.kps[b] = kps[b]; G.kpitch[b] = kpitch[b]; G.cnt[b] = cnt[b]; G.cap[b] = cap[b];
        G.prior[b] = prior[b];
    }
    for (int p = 0; p < npairs; p++) { G.qbin[p] = qbin[p]; G.tbin[p] = tbin[p]; }
    efx_guided_grid(radius, width, height, &G.g.x0, &G.g.y0, &G.g.edge, &G.g.gw, &G.g.gh);
    const int ncells = G.g.gw * G.g.gh;
    const size_t nb = (size_t)nbins, r = (size_t)(cap_max > 0 ? cap_max : 1);
    uint8_t* s = static_cast<uint8_t*>(scratch);
    auto take = [&s](size_t bytes) { uint8_t* p = s; s += align256(bytes); return p; };
    const size_t count_bytes = nb * (ncells + 1) * 4;
    G.count = reinterpret_cast<int*>(take(count_bytes));
    const int nblk = (ncells + 1 + GUIDED_SCAN_CELLS - 1) / GUIDED_SCAN_CELLS;
    G.wgsum = reinterpret_cast<int*>(take(nb * nblk * 4));
    G.start = reinterpret_cast<int*>(take(nb * (ncells + 2) * 4));
    G.cell = reinterpret_cast<int*>(take(nb * r * 4));
    G.rank = reinterpret_cast<int*>(take(nb * r * 4));
    G.sidx = reinterpret_cast<int*>(take(nb * r * 4));
    G.soct = reinterpret_cast<int*>(take(nb * r * 4));
    G.pred = reinterpret_cast<double2*>(take(nb * r * 16));
    G.spred = reinterpret_cast<double2*>(take(nb * r * 16));
    G.sdesc = take(nb * r * (size_t)desc_bytes);
    G.rows = (int)r;
    G.radius = radius; G.max_octave_diff = max_octave_diff; G.desc_bytes = desc_bytes;
    G.idx = static_cast<int*>(knn);
    G.dist = G.idx + (size_t)(2 * npairs) * 2 * r;
    G.cap_max = (int)r;
    hipError_t e = hipMemsetAsync(G.count, 0, count_bytes, stream);
    if (e != hipSuccess) return e;
    const dim3 rgrid((unsigned)((r + 255) / 256), 1, (unsigned)nbins);
    hipLaunchKernelGGL(guided_bin_kernel, rgrid, dim3(256), 0, stream, G);
    const dim3 cgrid((unsigned)nblk, 1, (unsigned)nbins);
    hipLaunchKernelGGL(guided_cellsum_kernel, cgrid, dim3(256), 0, stream, G, nblk);
    hipLaunchKernelGGL(guided_scan_kernel, cgrid, dim3(256), 0, stream, G, nblk);
    hipLaunchKernelGGL(guided_scatter_kernel, rgrid, dim3(256), 0, stream, G);
    const dim3 sgrid((unsigned)((r + 256 / GUIDED_LANES - 1) / (256 / GUIDED_LANES)), 1, (unsigned)(2 * npairs));
    if (desc_bytes == 32) hipLaunchKernelGGL(guided_search_kernel<8>, sgrid, dim3(256), 0, stream, G);
    else hipLaunchKernelGGL(guided_search_kernel<16>, sgrid, dim3(256), 0, stream, G);
    return hipGetLastError();
}
