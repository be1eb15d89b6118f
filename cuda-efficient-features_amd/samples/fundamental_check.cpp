// fundamental_check.cpp -- epipolar verification of an image sequence with parallax on the device without host round trips.  A
// sideways camera sees two texture layers at different depths: the upper half of every frame shows the far layer, the lower half
// the near one, and from frame to frame the layers move by different shifts along x.  The frames go through ONE batched
// detectAndCompute call, ONE batched mutual match of consecutive frames, ONE batched RANSAC homography call and ONE
// batched RANSAC fundamental-matrix call (S18) on the same device match lists; the host synchronises once, at the end.  A
// homography explains one layer, the epipolar model both: every pair must have a model from both calls, the fundamental inlier
// count must be at least 1.3 x the homography's, and the recovered F must put the true correspondences of both layers within one
// pixel (Sampson) of their epipolar lines.  Prints "fundamental ok" and returns 0 when every pair does.
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

static double sampson(const double* F, double x, double y, double u, double v)
{
    const double a = F[0] * x + F[1] * y + F[2], b = F[3] * x + F[4] * y + F[5], c = F[6] * x + F[7] * y + F[8];
    const double a2 = F[0] * u + F[3] * v + F[6], b2 = F[1] * u + F[4] * v + F[7];
    return std::fabs(a * u + b * v + c) / std::sqrt(a * a + b * b + a2 * a2 + b2 * b2);
}

#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    try {
        const int w = 1280, h = 720, nf = 7, cap = 4000, far_shift = 6, near_shift = 30, split = h / 2;
        const int sw = w + near_shift * nf;
        const std::vector<uint8_t> far_layer = synth(sw, h, 4242), near_layer = synth(sw, h, 2424);
        std::vector<std::vector<uint8_t>> img(nf, std::vector<uint8_t>((size_t)w * h));
        for (int f = 0; f < nf; f++)
            for (int y = 0; y < h; y++) {
                const std::vector<uint8_t>& layer = y < split ? far_layer : near_layer;
                memcpy(&img[f][(size_t)y * w], &layer[(size_t)y * sw + (size_t)f * (y < split ? far_shift : near_shift)], (size_t)w);
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
        const int np = nf - 1;
        int* d_counts = nullptr;
        efx_homography* d_hom = nullptr;
        efx_fundamental* d_fun = nullptr;
        REQUIRE(hipMalloc(&d_counts, (nf + np) * sizeof(int)) == hipSuccess);
        REQUIRE(hipMalloc(&d_hom, np * sizeof(efx_homography)) == hipSuccess);
        REQUIRE(hipMalloc(&d_fun, np * sizeof(efx_fundamental)) == hipSuccess);
        int* d_nmatches = d_counts + nf;
        std::vector<int*> counts(nf);
        for (int f = 0; f < nf; f++) counts[f] = d_counts + f;
        std::vector<efx::DeviceMatrix> kps, desc;
        feature->detectAndComputeBatchAsync(frames, kps, desc, counts);
        efx::BFMatcher matcher;
        std::vector<const efx::DeviceMatrix*> q, t, kq, kt, mp;
        std::vector<const int*> nq, nt, cm;
        std::vector<int*> nm;
        std::vector<efx_homography*> hres;
        std::vector<efx_fundamental*> fres;
        for (int f = 0; f < np; f++) {
            q.push_back(&desc[f]); t.push_back(&desc[f + 1]); nq.push_back(counts[f]); nt.push_back(counts[f + 1]);
            nm.push_back(d_nmatches + f); cm.push_back(d_nmatches + f);
            kq.push_back(&kps[f]); kt.push_back(&kps[f + 1]); hres.push_back(d_hom + f); fres.push_back(d_fun + f);
        }
        std::vector<efx::DeviceMatrix> matches, hmasks, fmasks;
        matcher.matchMutualBatchAsync(q, nq, t, nt, 32, matches, nm, 0.9);
        for (auto& m : matches) mp.push_back(&m);
        matcher.findHomographyBatchAsync(kq, kt, mp, cm, hres, hmasks);
        matcher.findFundamentalBatchAsync(kq, kt, mp, cm, fres, fmasks);
        REQUIRE(hipStreamSynchronize(nullptr) == hipSuccess);                   // the only synchronisation of the loop

        std::vector<int> hc(nf + np);
        std::vector<efx_homography> hr(np);
        std::vector<efx_fundamental> fr(np);
        REQUIRE(hipMemcpy(hc.data(), d_counts, hc.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess);
        REQUIRE(hipMemcpy(hr.data(), d_hom, hr.size() * sizeof(efx_homography), hipMemcpyDeviceToHost) == hipSuccess);
        REQUIRE(hipMemcpy(fr.data(), d_fun, fr.size() * sizeof(efx_fundamental), hipMemcpyDeviceToHost) == hipSuccess);
        double worst = 0.0, least = 1e9;
        int inliers = 0;
        for (int f = 0; f < np; f++) {
            const int k = hc[nf + f];
            const efx_homography& H = hr[f];
            const efx_fundamental& F = fr[f];
            REQUIRE(k > 100);
            REQUIRE(H.hypothesis >= 0 && F.hypothesis >= 0 && F.refined == 1);
            double big = 0.0;
            for (int i = 0; i < 9; i++) big = std::fabs(F.F[i]) > std::fabs(big) ? F.F[i] : big;
            REQUIRE(big == 1.0);
            std::vector<uint8_t> mk((size_t)matches[f].rows);
            REQUIRE(hipMemcpy(mk.data(), fmasks[f].data(), mk.size(), hipMemcpyDeviceToHost) == hipSuccess);
            int set = 0;
            for (size_t i = 0; i < mk.size(); i++) { REQUIRE(mk[i] <= 1 && (i < (size_t)k || mk[i] == 0)); set += mk[i]; }
            REQUIRE(set == F.ninliers);
            const double ratio = (double)F.ninliers / (double)H.ninliers;
            least = ratio < least ? ratio : least;
            REQUIRE(F.ninliers * 10 >= H.ninliers * 13);
            // the true motion: a point of frame f at (x, y) lies at (x - shift, y) in frame f + 1
            for (int y = 20; y < h; y += 40)
                for (int x = 60; x < w; x += 60) {
                    const double e = sampson(F.F, x, y, x - (y < split ? far_shift : near_shift), y);
                    worst = e > worst ? e : worst;
                    REQUIRE(e < 1.0);
                }
            inliers += F.ninliers;
        }
        for (auto* p : d_frames) (void)hipFree(p);
        (void)hipFree(d_counts);
        (void)hipFree(d_hom);
        (void)hipFree(d_fun);
        printf("fundamental ok: %d frames, %d pairs, %d inliers, least inlier ratio to the homography %.2f, worst epipolar error %.3f px\n",
               nf, np, inliers, least, worst);
        return 0;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 2;
    }
}
