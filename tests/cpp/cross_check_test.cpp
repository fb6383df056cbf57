// cross_check_test.cpp -- VisualOdometry::set_cross_check through the C++ facade
// (include/VisualOdometry.hpp): match_descriptors on one frame pair with the cross-check off, on and
// off again.  Prints the three match counts and the mutual pairs for tests/test_gpu_mutual_match.py;
// exits 1 if the mutual count differs from the expected one (the test's restatement), if the mutual
// pairs are no subsequence of the plain ones, or if switching back does not restore them.
//
// usage: vo_cross_check_test <frame1.pgm|png> <frame2.pgm|png> <expected mutual count>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "VisualOdometry.hpp"

using namespace vo_mi355x;

static std::vector<uint8_t> load(const char* path, int* w, int* h)
{
    check(vo_imread_gray(path, nullptr, 0, w, h), "vo_imread_gray");
    std::vector<uint8_t> px((size_t)*w * *h);
    check(vo_imread_gray(path, px.data(), px.size(), w, h), "vo_imread_gray");
    return px;
}

int main(int argc, char** argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <frame1> <frame2> <expected mutual count>\n", argv[0]);
        return 2;
    }
    const long expected = std::atol(argv[3]);
    int w1, h1, w2, h2;
    std::vector<uint8_t> a = load(argv[1], &w1, &h1), b = load(argv[2], &w2, &h2);
    VisualOdometry vo("", 8, w1, h1);
    auto [desc1, kpts1] = vo.compute_descriptor_with_key_points(GrayImage{a.data(), w1, h1, (size_t)w1});
    auto [desc2, kpts2] = vo.compute_descriptor_with_key_points(GrayImage{b.data(), w2, h2, (size_t)w2});
    if (vo.cross_check()) return 3;                           // off by default
    const auto plain = vo.match_descriptors(desc1, desc2);
    vo.set_cross_check(true);
    if (!vo.cross_check()) return 3;
    const auto mutual = vo.match_descriptors(desc1, desc2);
    vo.set_cross_check(false);
    const auto again = vo.match_descriptors(desc1, desc2);
    std::printf("plain %zu mutual %zu again %zu\n", plain.size(), mutual.size(), again.size());
    std::printf("pairs");
    for (const auto& p : mutual) std::printf(" %d %d", p.first, p.second);
    std::printf("\n");
    // a subsequence of the plain pairs, in their order
    size_t k = 0;
    for (const auto& p : mutual) {
        while (k < plain.size() && plain[k] != p) ++k;
        if (k == plain.size()) return 1;
        ++k;
    }
    if (again != plain) return 1;
    return (long)mutual.size() == expected ? 0 : 1;
}
