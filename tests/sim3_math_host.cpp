// Host build of the Sim3Solver kernels' arithmetic (sp-slam_amd/csrc/sim3_math.h) behind a C ABI, compiled by
// tests/test_sim3_solver_host.py with g++ -ffp-contract=off and held against tests/sim3_solver_ref.py bit for bit.
#include "../sp-slam_amd/csrc/sim3_math.h"

using namespace spslam::sim3;

extern "C" {

void sim3_host_draw3(const int32_t* r, int rand_max, int n, int* idx) { draw3(r, rand_max, n, idx); }

// X1, X2: three points of three floats each; out: s, R[9], t[3], T12[12], T21[12]
void sim3_host_hypothesis(const float* X1, const float* X2, int fix_scale, float* out) {
    float A[3][3], B[3][3];
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) {
            A[i][r] = X1[3 * i + r];
            B[i][r] = X2[3 * i + r];
        }
    JacobiHost J;
    compute_sim3(J, A, B, fix_scale != 0, out, out + 1, out + 10);
    transforms(out[0], out + 1, out + 10, out + 13, out + 25);
}

// corr: the 14 words of a Corr; cam: fx, fy, cx, cy
int sim3_host_inlier(const void* corr, const float* T12, const float* T21, const float* cam) {
    return is_inlier(*(const Corr*)corr, T12, T21, cam[0], cam[1], cam[2], cam[3]) ? 1 : 0;
}

}
