// A stand-alone program over the PnPsolver cases for a host sanitizer: it links the referee (tests/pnp_ref.cpp) and
// the host build of the kernels' arithmetic (tests/pnp_host.cpp over sp-slam_amd/csrc/pnp_math.h), runs every call of
// every case through both and compares every result record, inlier byte, best-mask byte and frame point.
//   python tools/pnp_dump_cases.py cases.bin
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tools/pnp_check_main.cpp tests/pnp_ref.cpp \
//       tests/pnp_host.cpp -o pnp_check && ./pnp_check cases.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/spslam_gpu.h"

extern "C" {
int pnp_ref_run(const float* cam, const float* sigma2, const void* keys_un, int n_frame, const int32_t* match,
                const int32_t* kf_rows, int n_kf, const float* xw, const uint8_t* bad, const int32_t* rnd,
                int rand_iterations, int rand_max, double probability, int min_inliers, int max_iterations, int min_set,
                float epsilon, float th2, int n_calls, const int32_t* n_iterations, void* results, uint8_t* inliers,
                uint8_t* best_mask, int32_t* frame_points, void* trace, int trace_cap, int32_t* counters);
int pnp_ref_sizes(int which);
int pnp_host_call(const float* cam, const float* sigma2, const spslam_keypoint* keys_un, int n_frame, const int32_t* match,
                  const int32_t* kf_rows, int n_kf, const float* xw, const uint8_t* bad, const int32_t* rnd, int rand_max,
                  const int32_t* max_its, const int32_t* min_n, int max_iterations, float th2,
                  const spslam_pnp_problem* Q, spslam_pnp_result* result, uint8_t* inliers, uint8_t* best_mask,
                  int32_t* frame_points, int32_t* hyp_out, int32_t* n_refines);
}

namespace {

struct Reader {
    FILE* f;
    template <class T> std::vector<T> vec(size_t n) {
        std::vector<T> v(n);
        if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short file\n"); std::exit(2); }
        return v;
    }
    template <class T> T one() { return vec<T>(1)[0]; }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: pnp_check cases.bin\n"); return 2; }
    Reader R{std::fopen(argv[1], "rb")};
    if (!R.f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    // header: n_rows, n_cases, rand_max, probability, th2; camera (4 floats), sigma2 (8 floats); xw, bad
    const int n_rows = R.one<int32_t>(), n_cases = R.one<int32_t>(), rand_max = R.one<int32_t>();
    const double probability = R.one<double>();
    const float th2 = R.one<float>();
    const std::vector<float> cam = R.vec<float>(4), sigma2 = R.vec<float>(8), xw = R.vec<float>(3 * (size_t)n_rows);
    const std::vector<uint8_t> bad = R.vec<uint8_t>(n_rows);
    int calls = 0, differ = 0;
    for (int c = 0; c < n_cases; c++) {
        // per case: n_frame, n_kf, rand_iterations, min_inliers, max_iterations, epsilon, n_calls, calls, then the arrays
        const int nf = R.one<int32_t>(), n_kf = R.one<int32_t>(), rand_iterations = R.one<int32_t>();
        const int min_inliers = R.one<int32_t>(), max_iterations = R.one<int32_t>();
        const float epsilon = R.one<float>();
        const int n_calls = R.one<int32_t>();
        const std::vector<int32_t> n_it = R.vec<int32_t>(n_calls);
        const std::vector<spslam_keypoint> kun = R.vec<spslam_keypoint>(nf);
        const std::vector<int32_t> match = R.vec<int32_t>(nf), kf_rows = R.vec<int32_t>(n_kf);
        const std::vector<int32_t> rnd = R.vec<int32_t>(4 * (size_t)rand_iterations);
        const size_t W = nf > 0 ? nf : 1;
        std::vector<spslam_pnp_result> want(n_calls);
        std::vector<uint8_t> w_inl(n_calls * W), w_mask(n_calls * W);
        std::vector<int32_t> w_fp(n_calls * W);
        std::vector<uint8_t> trace((size_t)pnp_ref_sizes(1) * 4096);
        int32_t counters[2];
        pnp_ref_run(cam.data(), sigma2.data(), kun.data(), nf, match.data(), kf_rows.data(), n_kf, xw.data(), bad.data(),
                    rnd.data(), rand_iterations, rand_max, probability, min_inliers, max_iterations, 4, epsilon, th2,
                    n_calls, n_it.data(), want.data(), w_inl.data(), w_mask.data(), w_fp.data(), trace.data(), 4096,
                    counters);
        std::vector<int32_t> max_its(W + 1), min_n(W + 1);
        // the tables come from the referee's own SetRansacParameters, one N at a time, through its result record:
        // here only the entry for this case's N is needed
        for (size_t n = 0; n <= W; n++) { max_its[n] = 0; min_n[n] = 1 << 30; }
        if (want[0].n <= (int)W) { max_its[want[0].n] = want[0].max_its; min_n[want[0].n] = want[0].min_inliers; }
        spslam_pnp_problem Q;
        std::memset(&Q, 0, sizeof Q);
        std::vector<uint8_t> mask(W, 0);
        for (int r = 0; r < n_calls; r++, calls++) {
            Q.n_iterations = n_it[r];
            Q.rand_iterations = rand_iterations;
            spslam_pnp_result got;
            std::vector<uint8_t> inl(W, 0);
            std::vector<int32_t> fp(W, -1), hyp(2 * (size_t)max_iterations);
            int32_t n_refines = 0;
            pnp_host_call(cam.data(), sigma2.data(), kun.data(), nf, match.data(), kf_rows.data(), n_kf, xw.data(),
                          bad.data(), rnd.data(), rand_max, max_its.data(), min_n.data(), max_iterations, th2, &Q, &got,
                          inl.data(), mask.data(), fp.data(), hyp.data(), &n_refines);
            const bool pose = got.status == SPSLAM_PNP_REFINED || got.status == SPSLAM_PNP_BEST_NO_MORE;
            bool same = std::memcmp(&got, &want[r], sizeof got) == 0 &&
                        std::memcmp(inl.data(), w_inl.data() + r * (size_t)nf, nf) == 0 &&
                        std::memcmp(mask.data(), w_mask.data() + r * (size_t)nf, nf) == 0;
            if (pose) same = same && std::memcmp(fp.data(), w_fp.data() + r * (size_t)nf, 4 * (size_t)nf) == 0;
            if (!same) { differ++; std::printf("case %d call %d differs\n", c, r); }
            Q.iterations_done = got.iterations_done;
            Q.best_inliers = got.best_inliers;
            std::memcpy(Q.best_Tcw, got.best_Tcw, sizeof Q.best_Tcw);
        }
    }
    std::fclose(R.f);
    std::printf("%d cases, %d calls, %d differ\n", n_cases, calls, differ);
    if (!differ) std::printf("all calls equal\n");
    return differ ? 1 : 0;
}
