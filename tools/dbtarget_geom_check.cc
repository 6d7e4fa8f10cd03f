// Stand-alone driver of the host geometry behind ocrvi_db_target_jobs (csrc/db_target_geom.h + csrc/clip_union.h) for sanitizer runs: the
// header reads polygons it did not make, so it is run here on seeded polygon families -- convex and star-shaped n-gons, fractional and
// duplicate vertices, thin strips, dumbbells, bow-ties, coordinates far outside the image -- with no Python and no GPU in the process.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I ocr_vi_invoice_amd/csrc \
//       tools/dbtarget_geom_check.cc -o build/dbtarget_geom_check && build/dbtarget_geom_check [polygons per family]
// Prints the job counts per kind; any sanitizer report ends the run with a non-zero status.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "db_target_geom.h"

int main(int argc, char** argv) {
    const int per_family = argc > 1 ? atoi(argv[1]) : 400;
    const int H = 160, W = 200;
    std::mt19937 rng(20240613);
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    auto rot = [](std::vector<float>& p, double ang, double cx, double cy) {
        for (size_t i = 0; i < p.size(); i += 2) {
            const double x = p[i], y = p[i + 1];
            p[i] = (float)(cx + x * cos(ang) - y * sin(ang));
            p[i + 1] = (float)(cy + x * sin(ang) + y * cos(ang));
        }
    };
    long long kinds[3] = {0, 0, 0}, points = 0, polygons = 0;
    for (int family = 0; family < 7; ++family) {
        std::vector<float> xy;
        std::vector<int32_t> offs{0};
        for (int k = 0; k < per_family; ++k) {
            const int n = 3 + (int)(rng() % 10);
            const double cx = uni(30, W - 30), cy = uni(30, H - 30);
            std::vector<double> ang(n);
            for (double& a : ang) a = uni(0, 6.283185307179586);
            std::sort(ang.begin(), ang.end());
            std::vector<float> p;
            switch (family) {
                case 0: {   // convex
                    const double rx = uni(4, 40), ry = uni(4, 40);
                    for (double a : ang) { p.push_back((float)(cx + rx * cos(a))); p.push_back((float)(cy + ry * sin(a))); }
                    break;
                }
                case 1:     // star-shaped, integer
                case 2:     // quarter-pixel with repeated vertices and a closing duplicate
                case 6: {   // three times the size around a centre that may lie outside the image
                    const double ex = family == 6 ? uni(-60, 60) : 0, ey = family == 6 ? uni(-70, 70) : 0, s = family == 6 ? 3 : 1;
                    for (double a : ang) {
                        const double r = uni(3, 40), x = cx + ex + s * r * cos(a), y = cy + ey + s * r * sin(a);
                        const double q = family == 1 ? 1 : 4;
                        p.push_back((float)(family == 6 ? x : floor(x * q + 0.5) / q));
                        p.push_back((float)(family == 6 ? y : floor(y * q + 0.5) / q));
                        if (family == 2 && rng() % 3 == 0) { p.push_back(p[p.size() - 2]); p.push_back(p[p.size() - 2]); }
                    }
                    if (family == 2 && rng() % 2) { p.push_back(p[0]); p.push_back(p[1]); }
                    break;
                }
                case 3: {   // thin strip
                    const double ln = uni(20, 150) / 2, wd = uni(0.5, 7) / 2;
                    p = {(float)-ln, (float)-wd, (float)ln, (float)-wd, (float)ln, (float)wd, (float)-ln, (float)wd};
                    rot(p, uni(0, 3.14159), cx, cy);
                    break;
                }
                case 4: {   // dumbbell
                    const int a = 10 + (int)(rng() % 30), nk = 4 + (int)(rng() % 26), nw = 1 + (int)(rng() % 7), y0 = (a - nw) / 2, y1 = y0 + nw;
                    const int d[24] = {0, 0, a, 0, a, y0, a + nk, y0, a + nk, 0, 2 * a + nk, 0, 2 * a + nk, a, a + nk, a, a + nk, y1, a, y1, a, a, 0, a};
                    for (int i = 0; i < 24; i += 2) { p.push_back((float)(d[i] - a)); p.push_back((float)(d[i + 1] - a / 2)); }
                    rot(p, rng() % 2 ? 0.0 : uni(0, 3.14159), cx, cy);
                    break;
                }
                default: {  // bow-tie
                    const double bw = uni(2, 60), bh = uni(2, 60);
                    p = {(float)-bw, (float)-bh, (float)bw, (float)bh, (float)bw, (float)-bh, (float)-bw, (float)bh};
                    rot(p, uni(0, 3.14159), cx, cy);
                }
            }
            xy.insert(xy.end(), p.begin(), p.end());
            offs.push_back((int32_t)(xy.size() / 2));
        }
        offs.push_back(offs.back() + 2);   // one polygon too short to count: its two vertices are never read
        xy.insert(xy.end(), {1.f, 1.f, 2.f, 2.f});
        dbtarget::ImageJobs out;
        dbtarget::image_jobs(family, H, W, xy.data(), offs.data(), (int)offs.size() - 1, 0.4, true, out);
        for (size_t j = 0; j < out.jobs.size(); j += dbtarget::kJobInts) {
            kinds[out.jobs[j + 1]]++;
            if (out.jobs[j + 3] <= out.jobs[j + 2] || (size_t)out.jobs[j + 3] > out.points.size() / 2) { printf("bad point range in family %d\n", family); return 1; }
        }
        points += (long long)out.points.size() / 2;
        polygons += per_family;
    }
    printf("%lld polygons -> %lld GT, %lld MASK, %lld THRESH jobs, %lld points\n", polygons, kinds[0], kinds[1], kinds[2], points);
    return kinds[0] + kinds[1] == polygons ? 0 : 1;
}
