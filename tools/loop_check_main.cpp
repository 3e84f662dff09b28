// Stand-alone run of the index checks behind the loop-closing entries' host forms (sp-slam_amd/csrc/loop_check.h) for
// a host sanitizer; it needs no device:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/loop_check_main.cpp -o loop_check
//   ./loop_check
// Every table is a heap vector of its exact size, so a check that reads one entry too many is reported.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../sp-slam_amd/csrc/loop_check.h"

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

// a keyframe of n keypoints, keypoint i in cell i of the grid, FeatureVector nodes of two features each
struct Keyframe {
    std::vector<uint8_t> desc, has;
    std::vector<spslam_keypoint> keys;
    std::vector<uint32_t> nodes;
    std::vector<int32_t> start, feats, grid_off, grid_idx, rows;
    float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int n;
    explicit Keyframe(int n_) : desc((size_t)n_ * 32), has(n_, 1), keys(n_), grid_off(kLoopGridCells + 1), grid_idx(n_),
                                rows(n_), n(n_) {
        start.push_back(0);
        for (int i = 0; i < n; i++) {
            feats.push_back(i);
            grid_idx[i] = i;
            rows[i] = i % 3 ? i : -1;
            if (i % 2 == 1 || i == n - 1) {
                nodes.push_back(10u * (uint32_t)nodes.size());
                start.push_back(i + 1);
            }
        }
        for (int c = 0; c <= kLoopGridCells; c++) grid_off[c] = c < n ? c : n;
    }
    spslam_bow_keyframe bow() const {
        return {desc.data(), keys.data(), has.data(), nodes.data(), start.data(), feats.data(), n, (int32_t)nodes.size()};
    }
    spslam_sim3_keyframe sim3() const {
        return {Tcw, keys.data(), desc.data(), grid_off.data(), grid_idx.data(), rows.data(), n, 0};
    }
};

}  // namespace

int main() {
    for (int n : {0, 1, 2, 7, 64}) {
        Keyframe k(n);
        const spslam_bow_keyframe b = k.bow();
        expect(loop_check_bow_keyframe(&b), nullptr, "a sound FeatureVector");
        const spslam_sim3_keyframe s = k.sim3();
        expect(loop_check_sim3_keyframe(&s, n), nullptr, "a sound Sim3 keyframe");
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), n), nullptr, "a sound grid");
        std::vector<spslam_local_point> pts(5);
        expect(loop_check_scw_problem(k.Tcw, pts.data(), 5, k.keys.data(), k.desc.data(), n, k.grid_off.data(),
                                      k.grid_idx.data()), nullptr, "a sound Scw problem");
        std::vector<int32_t> m(n, -1);
        if (n) m[n - 1] = n - 1;
        expect(loop_check_match12(m.data(), n, n), nullptr, "a sound match12");
    }
    {   // the FeatureVector
        Keyframe k(7);
        spslam_bow_keyframe b = k.bow();
        expect(loop_check_bow_keyframe(nullptr), "missing", "no keyframe");
        b.n = 8193;
        expect(loop_check_bow_keyframe(&b), "n outside", "n too large");
        b = k.bow();
        b.n_fv = 8;
        expect(loop_check_bow_keyframe(&b), "more nodes", "n_fv above n");
        b = k.bow();
        k.feats[3] = 7;
        expect(loop_check_bow_keyframe(&b), "outside the keypoints", "a feature == n");
        k.feats[3] = -1;
        expect(loop_check_bow_keyframe(&b), "outside the keypoints", "a negative feature");
        k.feats[3] = 3;
        k.nodes[1] = k.nodes[0];
        expect(loop_check_bow_keyframe(&b), "do not ascend", "equal nodes");
        k.nodes[1] = 10;
        k.start[2] = 1;
        expect(loop_check_bow_keyframe(&b), "descends", "fv_start descends");
        k.start[2] = 4;
        k.start.back() = 8;
        expect(loop_check_bow_keyframe(&b), "more features", "fv_start past n");
        k.start.back() = 7;
        k.start[0] = 1;
        expect(loop_check_bow_keyframe(&b), "begin at 0", "fv_start[0] != 0");
        k.start[0] = 0;
        b.fv_start = nullptr;
        expect(loop_check_bow_keyframe(&b), "fv_start is missing", "no fv_start");
        b = k.bow();
        b.has_point = nullptr;
        expect(loop_check_bow_keyframe(&b), "keypoint array", "no has_point");
        expect(loop_check_bow_keyframe(&(b = k.bow())), nullptr, "restored");
    }
    {   // the grid, the map points, match12
        Keyframe k(7);
        k.grid_idx[2] = 7;
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), 7), "grid entry outside", "a grid entry == n");
        k.grid_idx[2] = -1;
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), 7), "grid entry outside", "a negative grid entry");
        k.grid_idx[2] = 2;
        k.grid_off[3] = 1;
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), 7), "descends", "grid_off descends");
        k.grid_off[3] = 3;
        k.grid_off[kLoopGridCells] = 8;
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), 7), "more keypoints", "grid past n");
        k.grid_off[kLoopGridCells] = 7;
        k.grid_off[0] = 1;
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), 7), "begin at 0", "grid_off[0] != 0");
        k.grid_off[0] = 0;
        expect(loop_check_grid(nullptr, k.grid_idx.data(), 7), "grid_off is missing", "no grid_off");
        expect(loop_check_grid(k.grid_off.data(), nullptr, 7), "grid_idx is missing", "no grid_idx");
        expect(loop_check_grid(k.grid_off.data(), k.grid_idx.data(), -1), "n_kp outside", "negative n_kp");
        spslam_sim3_keyframe s = k.sim3();
        expect(loop_check_sim3_keyframe(&s, 5), "map point outside", "a row == n_rows");
        k.rows[1] = -2;
        expect(loop_check_sim3_keyframe(&s, 7), "map point outside", "a row below -1");
        k.rows[1] = 1;
        s.Tcw = nullptr;
        expect(loop_check_sim3_keyframe(&s, 7), "Tcw is missing", "no Tcw");
        s = k.sim3();
        s.match_row = nullptr;
        expect(loop_check_sim3_keyframe(&s, 7), "keypoint array", "no match_row");
        expect(loop_check_scw_problem(nullptr, nullptr, 0, k.keys.data(), k.desc.data(), 7, k.grid_off.data(),
                                      k.grid_idx.data()), "Scw is missing", "no Scw");
        expect(loop_check_scw_problem(k.Tcw, nullptr, 3, k.keys.data(), k.desc.data(), 7, k.grid_off.data(),
                                      k.grid_idx.data()), "points are missing", "no points");
        expect(loop_check_scw_problem(k.Tcw, nullptr, -1, k.keys.data(), k.desc.data(), 7, k.grid_off.data(),
                                      k.grid_idx.data()), "n_points outside", "negative n_points");
        expect(loop_check_scw_problem(k.Tcw, nullptr, 0, nullptr, k.desc.data(), 7, k.grid_off.data(),
                                      k.grid_idx.data()), "keypoint array", "no keys_un");
        std::vector<int32_t> m(7, -1);
        m[6] = 5;
        expect(loop_check_match12(m.data(), 7, 5), "match12 entry outside", "a match == n2");
        m[6] = -2;
        expect(loop_check_match12(m.data(), 7, 5), "match12 entry outside", "a match below -1");
        expect(loop_check_match12(nullptr, 7, 5), "match12 is missing", "no match12");
        expect(loop_check_match12(nullptr, 0, 5), nullptr, "no match12 and no keypoints");
    }
    {   // Sim3Solver: the keyframes (octaves against the levels), the call's parameters, the state and the draws
        for (int n : {0, 1, 7, 64}) {
            Keyframe k(n);
            const spslam_sim3_keyframe s = k.sim3();
            expect(loop_check_solver_keyframe(&s, n, 8), nullptr, "a sound solver keyframe");
        }
        Keyframe k(7);
        spslam_sim3_keyframe s = k.sim3();
        s.grid_off = nullptr; s.grid_idx = nullptr; s.desc = nullptr;   // not read by the solver
        expect(loop_check_solver_keyframe(&s, 7, 8), nullptr, "no grid and no descriptors");
        expect(loop_check_solver_keyframe(nullptr, 7, 8), "keyframe is missing", "no keyframe");
        expect(loop_check_solver_keyframe(&s, 5, 8), "map point outside", "a row == n_rows");
        k.rows[1] = -2;
        expect(loop_check_solver_keyframe(&s, 7, 8), "map point outside", "a row below -1");
        k.rows[1] = 1;
        k.keys[6].octave = 8;
        expect(loop_check_solver_keyframe(&s, 7, 8), "octave outside", "an octave == n_levels");
        expect(loop_check_solver_keyframe(&s, 7, 9), nullptr, "the octave inside nine levels");
        k.keys[6].octave = -1;
        expect(loop_check_solver_keyframe(&s, 7, 8), "octave outside", "a negative octave");
        k.keys[6].octave = 0;
        s.n = 8193;
        expect(loop_check_solver_keyframe(&s, 7, 8), "n outside", "n too large");
        s = k.sim3();
        s.Tcw = nullptr;
        expect(loop_check_solver_keyframe(&s, 7, 8), "Tcw is missing", "no Tcw");
        s = k.sim3();
        s.keys_un = nullptr;
        expect(loop_check_solver_keyframe(&s, 7, 8), "keypoint array", "no keys_un");

        spslam_sim3_solver_params P{20, 300, 2147483647, 1};
        std::vector<int32_t> draws(3 * 300, 5);
        draws.back() = 2147483647;
        int done = 0, best = 0;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), nullptr, "a sound call");
        expect(loop_check_solver_call(nullptr, 0.99, 5, &done, &best, draws.data()), "parameters are missing", "no parameters");
        P.min_inliers = 2;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "min_inliers below 3", "min_inliers 2");
        P.min_inliers = 3;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), nullptr, "min_inliers 3");
        P.max_iterations = 0;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "max_iterations outside", "no iterations");
        P.max_iterations = SPSLAM_SIM3_MAX_ITERATIONS + 1;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "max_iterations outside", "too many iterations");
        P.max_iterations = 300;
        P.rand_max = 0;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "rand_max below 1", "rand_max 0");
        P.rand_max = 2147483647;
        expect(loop_check_solver_call(&P, 1.0, 5, &done, &best, draws.data()), "probability outside", "probability 1");
        expect(loop_check_solver_call(&P, 0.99, -1, &done, &best, draws.data()), "n_iterations is negative", "n_iterations -1");
        expect(loop_check_solver_call(&P, 0.99, 0, &done, &best, draws.data()), nullptr, "n_iterations 0");
        expect(loop_check_solver_call(&P, 0.99, 5, nullptr, &best, draws.data()), "state is missing", "no state");
        done = -1;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "state is negative", "iterations_done -1");
        done = 0;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, nullptr), "draws are missing", "no draws");
        draws.back() = -1;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "draw outside", "a negative last draw");
        draws.back() = 7;
        P.rand_max = 6;
        expect(loop_check_solver_call(&P, 0.99, 5, &done, &best, draws.data()), "draw outside", "a draw above rand_max");
    }
    {   // OptimizeSim3: the parameters and the pair record (the keyframes are the solver's, match12 as above)
        spslam_sim3_opt_params P{10.f, 1, 20, 0};
        spslam_sim3_pair pair{};
        expect(loop_check_opt_call(&P, &pair), nullptr, "a sound OptimizeSim3 call");
        expect(loop_check_opt_call(nullptr, &pair), "parameters are missing", "no OptimizeSim3 parameters");
        expect(loop_check_opt_call(&P, nullptr), "pair is missing", "no pair");
        P.fix_scale = 0;
        expect(loop_check_opt_call(&P, &pair), "fix_scale is not 1", "fix_scale 0");
        P.fix_scale = 2;
        expect(loop_check_opt_call(&P, &pair), "fix_scale is not 1", "fix_scale 2");
        P.fix_scale = 1;
        P.th2 = 0.f;
        expect(loop_check_opt_call(&P, &pair), "th2 is not positive", "th2 0");
        P.th2 = -10.f;
        expect(loop_check_opt_call(&P, &pair), "th2 is not positive", "th2 -10");
        P.th2 = 0.f / 0.f;
        expect(loop_check_opt_call(&P, &pair), "th2 is not positive", "th2 NaN");
        P.th2 = 1e-30f;
        expect(loop_check_opt_call(&P, &pair), nullptr, "a tiny th2");
    }
    if (failures) return 1;
    std::printf("loop_check: all checks hold\n");
    return 0;
}
