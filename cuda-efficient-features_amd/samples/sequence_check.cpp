// sequence_check.cpp -- the loop of samples/sample_image_sequence.cpp:70-137 on the device without host round trips: a synthetic
// sequence (one scene drifting by a few pixels per frame) goes through ONE batched detectAndCompute call, then the mutual
// ratio-test matches of every pair of consecutive frames through ONE batched matcher call fed by the device keypoint counts; the
// host synchronises once, at the end.  The result is checked against the sample's own filter run on the host over knnMatch
// results in both directions.  Prints "sequence ok" and returns 0 when every pair agrees.
#include "../host/efficient_features.hpp"

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

#define REQUIRE(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    try {
        const int w = 1280, h = 720, nf = 17, pad = 64, cap = 4000;
        const std::vector<uint8_t> scene = synth(w + pad, h + pad, 777);
        std::vector<uint8_t*> d_frames(nf);
        std::vector<efx::DeviceImage> frames(nf);
        for (int f = 0; f < nf; f++) {                      // frame f: the scene's window at (3 f, 2 f)
            REQUIRE(hipMalloc(&d_frames[f], (size_t)w * h) == hipSuccess);
            REQUIRE(hipMemcpy2D(d_frames[f], w, scene.data() + (size_t)(2 * f) * (w + pad) + 3 * f, w + pad, w, h, hipMemcpyHostToDevice) == hipSuccess);
            frames[f] = efx::DeviceImage{ d_frames[f], h, w, (size_t)w };
        }
        auto feature = efx::EfficientFeatures::create(cap);
        feature->setDescriptorType(efx::EfficientFeatures::BAD_256);
        int* d_counts = nullptr;
        REQUIRE(hipMalloc(&d_counts, (nf + nf - 1) * sizeof(int)) == hipSuccess);
        int* d_nmatches = d_counts + nf;
        std::vector<int*> counts(nf);
        for (int f = 0; f < nf; f++) counts[f] = d_counts + f;
        std::vector<efx::DeviceMatrix> kps, desc;
        feature->detectAndComputeBatchAsync(frames, kps, desc, counts);
        efx::BFMatcher matcher;
        std::vector<const efx::DeviceMatrix*> q, t;
        std::vector<const int*> nq, nt;
        std::vector<int*> nm;
        for (int f = 0; f + 1 < nf; f++) {
            q.push_back(&desc[f]); t.push_back(&desc[f + 1]); nq.push_back(counts[f]); nt.push_back(counts[f + 1]); nm.push_back(d_nmatches + f);
        }
        std::vector<efx::DeviceMatrix> matches;
        matcher.matchMutualBatchAsync(q, nq, t, nt, 32, matches, nm, 0.9);
        REQUIRE(hipStreamSynchronize(nullptr) == hipSuccess);                   // the only synchronisation of the loop

        std::vector<int> hc(nf + nf - 1);
        REQUIRE(hipMemcpy(hc.data(), d_counts, hc.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess);
        efx::BFMatcher knn;
        int total = 0;
        for (int f = 0; f + 1 < nf; f++) {
            const int n1 = hc[f], n2 = hc[f + 1], k = hc[nf + f];
            REQUIRE(n1 > 100 && n2 > 100);
            std::vector<int> got((size_t)3 * k);
            if (k > 0) REQUIRE(hipMemcpy(got.data(), matches[f].data(), got.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
            // the sample's filter (sample_image_sequence.cpp:114-137) on the host, over knnMatch in both directions
            std::vector<std::vector<efx::DMatch>> m12, m21;
            knn.knnMatch(desc[f], n1, desc[f + 1], n2, 32, m12);
            knn.knnMatch(desc[f + 1], n2, desc[f], n1, 32, m21);
            const double uniqueness = 0.9;
            std::vector<int> want;
            for (const auto& a : m12) {
                const auto& b = m21[a[0].trainIdx];
                if (a.size() > 1 && (double)a[0].distance > uniqueness * (double)a[1].distance) continue;
                if (b.size() > 1 && (double)b[0].distance > uniqueness * (double)b[1].distance) continue;
                if (b[0].trainIdx != a[0].queryIdx) continue;
                want.insert(want.end(), { a[0].queryIdx, a[0].trainIdx, a[0].distance });
            }
            REQUIRE(got == want);
            REQUIRE(k > n1 / 4);                            // consecutive frames of one scene: a good share matches
            total += k;
        }
        for (auto* p : d_frames) (void)hipFree(p);
        (void)hipFree(d_counts);
        printf("sequence ok: %d frames, %d pairs, %d mutual matches, equal to the host-side filter\n", nf, nf - 1, total);
        return 0;
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 2;
    }
}
