// guided_check.cpp -- the closed loop match -> H -> guided re-match -> H on the device without host round trips: frames rendered from
// one synthetic scene through known homographies go through ONE batched detectAndCompute call, ONE batched mutual match of
// consecutive frames, ONE batched RANSAC homography call, ONE batched guided match whose priors are the homography
// records the previous call left on the device, and ONE more homography call on the guided matches; the host synchronises once, at
// the end.  Every guided match must lie in the window around its prior's prediction, the guided matches must include every inlier
// of the first pass, and every second-pass model must map the frame corners within 2 pixels of the true homography.  Prints
// "guided ok" and returns 0 when every pair does.
#include "../host/efficient_features.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static std::vector<uint8_t> synth(int w, int h, uint32_t seed)
{
    std::vector<uint8_t> img((size_t)w * h, 128);
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int i = 0; i < (int)(700.0 * w * h / 1e6); i++) {
        const int sc[5] = { 10, 18, 32, 56, 96 };
        const int s = sc[rnd() % 5];
        const int rw = s / 2 + (int)(rnd() % (unsigned)s), rh = s / 2 + (int)(rnd() % (unsigned)s);
        const int x0 = (int)(rnd() % (unsigned)w), y0 = (int)(rnd() % (unsigned)h);
        const uint8_t v = (uint8_t)(rnd() & 255);
        for (int y = y0; y < y0 + rh && y < h; y++) memset(&img[(size_t)y * w + x0], v, (size_t)((x0 + rw < w ? rw : w - x0)));
    }
    for (auto& p : img) { const int v = (int)p + (int)(rnd() % 7) - 3; p = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
    return img;
}

struct M3 { double a[9]; };
static M3 mul(const M3& x, const M3& y)
{
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.a[3 * i + j] = x.a[3 * i] * y.a[j] + x.a[3 * i + 1] * y.a[3 + j] + x.a[3 * i + 2] * y.a[6 + j];
    return r;
}
static M3 inv(const M3& m)
{
    const double* a = m.a;
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double d = a[0] * c0 + a[1] * c1 + a[2] * c2;
    M3 r = { { c0 / d, (a[2] * a[7] - a[1] * a[8]) / d, (a[1] * a[5] - a[2] * a[4]) / d,
               c1 / d, (a[0] * a[8] - a[2] * a[6]) / d, (a[2] * a[3] - a[0] * a[5]) / d,
               c2 / d, (a[1] * a[6] - a[0] * a[7]) / d, (a[0] * a[4] - a[1] * a[3]) / d } };
    return r;
}
static void apply(const double* H, double x, double y, double& u, double& v)
{
    const double w = H[6] * x + H[7] * y + H[8];
    u = (H[0] * x + H[1] * y + H[2]) / w;
    v = (H[3] * x + H[4] * y + H[5]) / w;
}

#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    try {
        const int w = 1280, h = 720, sw = 1800, sh = 1200, nf = 9, cap = 4000;
        const std::vector<uint8_t> scene = synth(sw, sh, 4242);
        // G_f: scene -> frame f; frame f samples the scene bilinearly at G_f^-1 (u, v)
        std::vector<M3> G(nf);
        std::vector<std::vector<uint8_t>> img(nf, std::vector<uint8_t>((size_t)w * h));
        for (int f = 0; f < nf; f++) {
            const double th = 0.035 * (f % 3) - 0.02 * (f / 3), s = 1.0 + 0.03 * ((f % 4) - 1.5) / 1.5;
            const double px = 1.5e-5 * ((f % 2) ? 1 : -1), py = 1.0e-5 * (f % 3 - 1);
            const M3 toc = { { 1, 0, -0.5 * sw, 0, 1, -0.5 * sh, 0, 0, 1 } };
            const M3 rs = { { s * cos(th), -s * sin(th), 8.0 * f, s * sin(th), s * cos(th), -5.0 * f, px, py, 1 } };
            const M3 tof = { { 1, 0, 0.5 * w, 0, 1, 0.5 * h, 0, 0, 1 } };
            G[f] = mul(tof, mul(rs, toc));
            const M3 Gi = inv(G[f]);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    double sx, sy;
                    apply(Gi.a, x, y, sx, sy);
                    const int x0 = (int)floor(sx), y0 = (int)floor(sy);
                    double v = 128.0;
                    if (x0 >= 0 && y0 >= 0 && x0 + 1 < sw && y0 + 1 < sh) {
                        const double fx = sx - x0, fy = sy - y0;
                        const uint8_t* r0 = &scene[(size_t)y0 * sw + x0];
                        const uint8_t* r1 = r0 + sw;
                        v = (1 - fy) * ((1 - fx) * r0[0] + fx * r0[1]) + fy * ((1 - fx) * r1[0] + fx * r1[1]);
                    }
                    img[f][(size_t)y * w + x] = (uint8_t)(v + 0.5);
                }
        }
        std::vector<uint8_t*> d_frames(nf);
        std::vector<efx::DeviceImage> frames(nf);
        for (int f = 0; f < nf; f++) {
            REQUIRE(hipMalloc(&d_frames[f], (size_t)w * h) == hipSuccess);
            REQUIRE(hipMemcpy(d_frames[f], img[f].data(), (size_t)w * h, hipMemcpyHostToDevice) == hipSuccess);
            frames[f] = efx::DeviceImage{ d_frames[f], h, w, (size_t)w };
        }
        auto feature = efx::EfficientFeatures::create(cap);
        feature->setDescriptorType(efx::EfficientFeatures::BAD_256);
        int* d_counts = nullptr;
        efx_homography* d_res = nullptr;
        const int np = nf - 1;
        REQUIRE(hipMalloc(&d_counts, (nf + 2 * np) * sizeof(int)) == hipSuccess);
        REQUIRE(hipMalloc(&d_res, 2 * np * sizeof(efx_homography)) == hipSuccess);
        int* d_nmatches = d_counts + nf;
        std::vector<int*> counts(nf);
        for (int f = 0; f < nf; f++) counts[f] = d_counts + f;
        std::vector<efx::DeviceMatrix> kps, desc;
        feature->detectAndComputeBatchAsync(frames, kps, desc, counts);
        efx::BFMatcher matcher;
        std::vector<const efx::DeviceMatrix*> q, t, kq, kt, mp, gp;
        std::vector<const int*> nq, nt, cm, cg;
        std::vector<int*> nm, ng;
        std::vector<efx_homography*> res, res2;
        std::vector<const efx_homography*> prior;
        for (int f = 0; f < np; f++) {
            q.push_back(&desc[f]); t.push_back(&desc[f + 1]); nq.push_back(counts[f]); nt.push_back(counts[f + 1]);
            nm.push_back(d_nmatches + f); cm.push_back(d_nmatches + f);
            ng.push_back(d_nmatches + np + f); cg.push_back(d_nmatches + np + f);
            kq.push_back(&kps[f]); kt.push_back(&kps[f + 1]); res.push_back(d_res + f); res2.push_back(d_res + np + f);
            prior.push_back(d_res + f);
        }
        efx_guided_params gpar;
        efx_default_guided_params(&gpar);
        gpar.radius = 8.0f; gpar.width = w; gpar.height = h;
        std::vector<efx::DeviceMatrix> matches, masks, gmatches, gmasks;
        matcher.matchMutualBatchAsync(q, nq, t, nt, 32, matches, nm, 0.9);
        for (auto& m : matches) mp.push_back(&m);
        matcher.findHomographyBatchAsync(kq, kt, mp, cm, res, masks);
        matcher.matchGuidedBatchAsync(q, nq, kq, t, nt, kt, 32, prior, gmatches, ng, &gpar);
        for (auto& m : gmatches) gp.push_back(&m);
        matcher.findHomographyBatchAsync(kq, kt, gp, cg, res2, gmasks);
        REQUIRE(hipStreamSynchronize(nullptr) == hipSuccess);                   // the only synchronisation of the loop

        std::vector<int> hc(nf + 2 * np);
        std::vector<efx_homography> hr(2 * np);
        REQUIRE(hipMemcpy(hc.data(), d_counts, hc.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess);
        REQUIRE(hipMemcpy(hr.data(), d_res, hr.size() * sizeof(efx_homography), hipMemcpyDeviceToHost) == hipSuccess);
        std::vector<std::vector<int>> loc(nf, std::vector<int>((size_t)cap));
        for (int f = 0; f < nf; f++) REQUIRE(hipMemcpy(loc[f].data(), kps[f].data(), (size_t)cap * 4, hipMemcpyDeviceToHost) == hipSuccess);
        double worst = 0.0;
        int brute = 0, guided = 0, inliers = 0;
        for (int f = 0; f < np; f++) {
            const int k1 = hc[nf + f], k2 = hc[nf + np + f];
            const efx_homography& r1 = hr[f];
            const efx_homography& r2 = hr[np + f];
            REQUIRE(k1 > 100 && r1.hypothesis >= 0);
            REQUIRE(k2 >= r1.ninliers && k2 <= hc[f]);                          // an inlier (3 px) passes the 8 px window
            REQUIRE(r2.hypothesis >= 0 && r2.refined == 1 && r2.ninliers > k2 / 2 && r2.H[8] == 1.0);
            std::vector<int> gm((size_t)3 * k2);
            REQUIRE(hipMemcpy(gm.data(), gmatches[f].data(), gm.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
            for (int i = 0; i < k2; i++) {
                const int qi = gm[3 * i], ti = gm[3 * i + 1];
                REQUIRE(qi >= 0 && qi < hc[f] && ti >= 0 && ti < hc[f + 1] && (i == 0 || qi > gm[3 * i - 3]));
                double u, v;
                apply(r1.H, (double)(short)(loc[f][qi] & 0xffff), (double)(short)(loc[f][qi] >> 16), u, v);
                REQUIRE(std::fabs((double)(short)(loc[f + 1][ti] & 0xffff) - u) <= 8.0);
                REQUIRE(std::fabs((double)(short)(loc[f + 1][ti] >> 16) - v) <= 8.0);
            }
            const M3 truth = mul(G[f + 1], inv(G[f]));
            const double cx[4] = { 0, (double)w, (double)w, 0 }, cy[4] = { 0, 0, (double)h, (double)h };
            for (int c = 0; c < 4; c++) {
                double u0, v0, u1, v1;
                apply(truth.a, cx[c], cy[c], u0, v0);
                apply(r2.H, cx[c], cy[c], u1, v1);
                const double e = std::hypot(u1 - u0, v1 - v0);
                worst = e > worst ? e : worst;
                REQUIRE(e < 2.0);
            }
            brute += k1; guided += k2; inliers += r2.ninliers;
        }
        for (auto* p : d_frames) (void)hipFree(p);
        (void)hipFree(d_counts);
        (void)hipFree(d_res);
        printf("guided ok: %d frames, %d pairs, %d brute-force matches, %d guided matches, %d inliers, worst corner error %.3f px\n", nf, np,
               brute, guided, inliers, worst);
        return 0;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 2;
    }
}
