// Stand-alone run of the index checks behind the covisibility entries' host forms (sp-slam_amd/csrc/covis_check.h)
// for a host sanitizer; it needs no device:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/covis_check_main.cpp -o covis_check
//   ./covis_check
// Every table is a heap vector of its exact size, so a check that reads one entry too many is reported.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sp-slam_amd/csrc/covis_check.h"

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
    std::vector<int32_t> match_off, match_row, obs_off, obs_kf, obs_kp, kf_slot;
    std::vector<uint8_t> bad;
    std::vector<spslam_local_point> points;
    spslam_covis_map map() const {
        spslam_covis_map m{};
        m.match_off = match_off.data();
        m.match_row = match_row.empty() ? nullptr : match_row.data();
        m.obs_off = obs_off.data();
        m.obs_kf = obs_kf.empty() ? nullptr : obs_kf.data();
        m.obs_kp = obs_kp.empty() ? nullptr : obs_kp.data();
        m.kf_slot = kf_slot.data();
        m.point_bad = bad.empty() ? nullptr : bad.data();
        m.points = points.empty() ? nullptr : points.data();
        return m;
    }
};

// n_kf keyframes of kp keypoints; point r is seen by keyframes r % n_kf and (r + 1) % n_kf
Tables make(int n_kf, int kp) {
    Tables t;
    const int n_rows = n_kf * kp / 2;
    std::vector<std::vector<int>> matches(n_kf);
    t.obs_off.push_back(0);
    for (int r = 0; r < n_rows; r++) {
        int a = r % n_kf, b = (r + 1) % n_kf;
        if (a > b) std::swap(a, b);
        for (int k = a; k <= b; k += std::max(b - a, 1)) {  // a, then b when it is another keyframe
            t.obs_kf.push_back(k);
            t.obs_kp.push_back((int)matches[k].size());
            matches[k].push_back(r);
        }
        t.obs_off.push_back((int)t.obs_kf.size());
    }
    t.match_off.push_back(0);
    for (int k = 0; k < n_kf; k++) {
        matches[k].push_back(-1);
        t.match_row.insert(t.match_row.end(), matches[k].begin(), matches[k].end());
        t.match_off.push_back((int)t.match_row.size());
        t.kf_slot.push_back(n_kf - 1 - k);
    }
    t.bad.assign(n_rows, 0);
    t.points.assign(n_rows, spslam_local_point{});
    return t;
}

}  // namespace

int main() {
    for (int n_kf : {1, 2, 7, 1024}) {
        const int kp = n_kf == 1024 ? 4 : 10;
        const Tables t = make(n_kf, kp);
        const int n_rows = (int)t.bad.size(), cap = kp + 2;
        expect(covis_check_map(t.map(), n_kf, n_rows, false, 0, 0), nullptr, "sound map");
        expect(covis_check_map(t.map(), n_kf, n_rows, true, cap, n_kf), nullptr, "sound culling map");
        expect(covis_check_map(t.map(), n_kf, n_rows, true, cap, n_kf - 1), "slot outside", "too few slots");
        expect(covis_check_map(t.map(), 0, n_rows, false, 0, 0), "n_kf outside", "n_kf 0");
        expect(covis_check_map(t.map(), 1025, n_rows, false, 0, 0), "n_kf outside", "n_kf 1025");
        if (n_rows) {
            Tables u = t;
            u.match_row[0] = n_rows;
            expect(covis_check_map(u.map(), n_kf, n_rows, false, 0, 0), "match row outside", "row == n_rows");
            u = t;
            u.match_row.back() = -2;
            expect(covis_check_map(u.map(), n_kf, n_rows, false, 0, 0), "match row outside", "row -2");
            u = t;
            u.obs_kf.back() = n_kf;
            expect(covis_check_map(u.map(), n_kf, n_rows, false, 0, 0), "observer outside", "observer == n_kf");
            u = t;
            u.obs_kp[0] = cap;
            expect(covis_check_map(u.map(), n_kf, n_rows, true, cap, n_kf), "keypoint outside", "keypoint == cap");
            expect(covis_check_map(t.map(), n_kf, n_rows, true, 1, n_kf), "longer than cap", "cap 1");
            u = t;
            u.obs_off[1] = u.obs_off.back() + 1;
            expect(covis_check_map(u.map(), n_kf, n_rows, false, 0, 0), "decrease", "offsets decrease");
        }
        Tables u = t;
        u.match_off[0] = 1;
        expect(covis_check_map(u.map(), n_kf, n_rows, false, 0, 0), "start at 0", "offsets from 1");
        std::vector<int32_t> cand;
        for (int q = 0; q < n_kf; q++) cand.push_back(n_kf - 1 - q);
        expect(covis_check_candidates(cand.data(), n_kf, n_kf), nullptr, "sound candidates");
        expect(covis_check_candidates(nullptr, 0, n_kf), nullptr, "no candidates");
        cand[0] = n_kf;
        expect(covis_check_candidates(cand.data(), n_kf, n_kf), "candidate outside", "candidate == n_kf");
        expect(covis_check_candidates(cand.data(), 1025, n_kf), "too long", "1025 candidates");
        std::vector<int32_t> rows;
        for (int r = 0; r < n_rows; r++) rows.push_back(n_rows - 1 - r);
        expect(covis_check_rows(rows.data(), n_rows, n_rows), nullptr, "sound rows");
        expect(covis_check_rows(nullptr, 0, 0), nullptr, "no rows");
        if (n_rows) {
            rows[n_rows / 2] = n_rows;
            expect(covis_check_rows(rows.data(), n_rows, n_rows), "listed row outside", "row == n_rows");
        }
    }
    int32_t one = 0;
    uint8_t flag = 0;
    spslam_covis_graph g{&one, &one, &one, &one, &one, &one, &flag, 4, 0};
    expect(covis_check_graph(g, 4), nullptr, "sound graph");
    expect(covis_check_graph(g, 5), "stride", "stride below n_kf");
    g.covis = nullptr;
    expect(covis_check_graph(g, 4), "missing", "graph array missing");
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("covis_check: all checks hold\n");
    return failures != 0;
}
