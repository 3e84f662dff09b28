// Stand-alone run of the index checks behind the place-recognition entries' host forms
// (sp-slam_amd/csrc/place_check.h) for a host sanitizer; it needs no device:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/place_check_main.cpp -o place_check
//   ./place_check
// Every table is a heap vector of its exact size, so a check that reads one entry too many is reported.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sp-slam_amd/csrc/place_check.h"

using namespace spslam;

namespace {

int failures = 0;

void expect(const char* got, const char* want_part, const char* what) {
    const bool ok = want_part ? (got && std::strstr(got, want_part)) : got == nullptr;
    if (!ok) {
        std::printf("FAIL %s: got '%s', want '%s'\n", what, got ? got : "(sound)", want_part ? want_part : "(sound)");
        failures++;
    }
}

struct Tables {
    std::vector<uint32_t> words;
    std::vector<double> values;
    std::vector<int> n_bow;
    std::vector<uint8_t> in_db;
    std::vector<int32_t> covis, ordered, n_ordered;
    int cap = 0, stride = 0;
    spslam_place_db db() const {
        spslam_place_db d{};
        d.bow_words = words.data();
        d.bow_values = values.data();
        d.n_bow = n_bow.data();
        d.in_db = in_db.data();
        d.cap = cap;
        return d;
    }
    spslam_covis_graph graph() const {
        spslam_covis_graph g{};
        g.covis = const_cast<int32_t*>(covis.data());
        g.ordered = const_cast<int32_t*>(ordered.data());
        g.n_ordered = const_cast<int32_t*>(n_ordered.data());
        g.stride = stride;
        return g;
    }
};

// n_kf keyframes; keyframe k has (k * 7) % (cap + 1) words, so that 0 and cap occur
Tables make(int n_kf, int cap) {
    Tables t;
    t.cap = cap;
    t.stride = n_kf;
    t.words.assign((size_t)n_kf * cap, 0);
    t.values.assign((size_t)n_kf * cap, 0.5);
    for (int k = 0; k < n_kf; k++) {
        const int n = k == n_kf - 1 ? cap : (k * 7) % (cap + 1);
        t.n_bow.push_back(n);
        for (int i = 0; i < n; i++) t.words[(size_t)k * cap + i] = 3u * i + k;
        t.in_db.push_back(k & 1);
        for (int r = 0; r < SPSLAM_COVIS_BEST; r++) t.covis.push_back(r < 3 ? (k + r) % n_kf : -1);
        t.n_ordered.push_back(n_kf);
        for (int q = 0; q < n_kf; q++) t.ordered.push_back(n_kf - 1 - q);
    }
    return t;
}

}  // namespace

int main() {
    for (int n_kf : {1, 2, 9, 1024}) {
        const int cap = n_kf == 1024 ? 16 : 70;
        const Tables t = make(n_kf, cap);
        expect(place_check_db(t.db(), n_kf), nullptr, "sound database");
        expect(place_check_db(t.db(), 0), "n_kf outside", "n_kf 0");
        expect(place_check_db(t.db(), 1025), "n_kf outside", "n_kf 1025");
        Tables u = t;
        u.cap = 0;
        expect(place_check_db(u.db(), n_kf), "cap outside", "cap 0");
        u.cap = SPSLAM_PLACE_MAX_WORDS + 1;
        expect(place_check_db(u.db(), n_kf), "cap outside", "cap 8193");
        u = t;
        u.n_bow[n_kf - 1] = cap + 1;
        expect(place_check_db(u.db(), n_kf), "longer than cap", "n_bow == cap + 1");
        u.n_bow[n_kf - 1] = -1;
        expect(place_check_db(u.db(), n_kf), "longer than cap", "n_bow -1");
        u = t;
        u.words[(size_t)(n_kf - 1) * cap + cap - 1] = u.words[(size_t)(n_kf - 1) * cap + cap - 2];
        expect(place_check_db(u.db(), n_kf), "do not ascend", "a repeated last word");
        spslam_place_db d = t.db();
        d.in_db = nullptr;
        expect(place_check_db(d, n_kf), "missing", "in_db missing");

        expect(place_check_covis(t.covis.data(), n_kf), nullptr, "sound covis");
        expect(place_check_covis(nullptr, n_kf), "missing", "covis missing");
        u = t;
        u.covis.back() = n_kf;
        expect(place_check_covis(u.covis.data(), n_kf), "neighbour outside", "last neighbour == n_kf");
        u.covis.back() = -2;
        expect(place_check_covis(u.covis.data(), n_kf), "neighbour outside", "last neighbour -2");

        expect(place_check_query(t.graph(), n_kf, n_kf - 1), nullptr, "sound query");
        expect(place_check_query(t.graph(), n_kf, n_kf), "query outside", "query == n_kf");
        expect(place_check_query(t.graph(), n_kf, -1), "query outside", "query -1");
        u = t;
        u.stride = n_kf - 1;
        expect(place_check_query(u.graph(), n_kf, 0), "stride", "stride below n_kf");

        expect(place_check_ordered(t.graph(), n_kf, n_kf - 1), nullptr, "sound ordered list");
        u = t;
        u.ordered.back() = n_kf;
        expect(place_check_ordered(u.graph(), n_kf, n_kf - 1), "ordered keyframe outside", "last entry == n_kf");
        u.ordered.back() = -1;
        expect(place_check_ordered(u.graph(), n_kf, n_kf - 1), "ordered keyframe outside", "last entry -1");
        u = t;
        u.n_ordered[n_kf - 1] = n_kf + 1;
        expect(place_check_ordered(u.graph(), n_kf, n_kf - 1), "longer than its row", "n_ordered == stride + 1");
        u.n_ordered[n_kf - 1] = -1;
        expect(place_check_ordered(u.graph(), n_kf, n_kf - 1), "longer than its row", "n_ordered -1");
        u.n_ordered[n_kf - 1] = 0;
        expect(place_check_ordered(u.graph(), n_kf, n_kf - 1), nullptr, "an empty ordered list");
    }
    std::vector<uint32_t> w{1, 5, 9};
    std::vector<double> v{0.2, 0.3, 0.5};
    expect(place_check_vector(w.data(), v.data(), 3, 3), nullptr, "sound query vector");
    expect(place_check_vector(nullptr, nullptr, 0, SPSLAM_PLACE_MAX_WORDS), nullptr, "empty query vector");
    expect(place_check_vector(w.data(), v.data(), 3, 2), "longer than cap", "query longer than cap");
    expect(place_check_vector(w.data(), nullptr, 3, 3), "lacks", "values missing");
    w[2] = 5;
    expect(place_check_vector(w.data(), v.data(), 3, 3), "do not ascend", "query words repeat");
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("place_check: all checks hold\n");
    return failures != 0;
}
