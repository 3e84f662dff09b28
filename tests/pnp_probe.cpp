// The squared reprojection error that PnPsolver's inlier test compares with its bound, stated on the types the
// reference has it on -- a double rotation and translation, a double camera, float points, float camera coordinates
// and reciprocal depth, double projected pixel, float differences and result -- with the same association, and no
// contraction written out.  tests/test_pnp_host.py builds this with g++ -O3 -march=x86-64-v3 -ffp-contract=fast,
// the reference's -O3 -march=native on an FMA host, and holds pnp_math.h's written-out contractions against what the
// compiler makes of it.
struct Pose { double rot[3][3], trans[3]; };
struct Pinhole { double fx, fy, cx, cy; };
struct World { float x, y, z; };
struct Pixel { float u, v; };

static float squared_error(const Pose& T, const Pinhole& K, const World& w, const Pixel& seen) {
    float cam_x = T.rot[0][0] * w.x + T.rot[0][1] * w.y + T.rot[0][2] * w.z + T.trans[0];
    float cam_y = T.rot[1][0] * w.x + T.rot[1][1] * w.y + T.rot[1][2] * w.z + T.trans[1];
    float inv_depth = 1 / (T.rot[2][0] * w.x + T.rot[2][1] * w.y + T.rot[2][2] * w.z + T.trans[2]);
    double proj_u = K.cx + K.fx * cam_x * inv_depth;
    double proj_v = K.cy + K.fy * cam_y * inv_depth;
    float off_u = seen.u - proj_u;
    float off_v = seen.v - proj_v;
    return off_u * off_u + off_v * off_v;
}

extern "C" void pnp_probe_error2(int n, const float* xw, const float* uv, const double* Rt, const float* cam, float* out) {
    Pose T;
    for (int i = 0; i < 9; i++) T.rot[i / 3][i % 3] = Rt[i];
    for (int i = 0; i < 3; i++) T.trans[i] = Rt[9 + i];
    const Pinhole K{cam[0], cam[1], cam[2], cam[3]};
    for (int i = 0; i < n; i++)
        out[i] = squared_error(T, K, World{xw[3 * i], xw[3 * i + 1], xw[3 * i + 2]}, Pixel{uv[2 * i], uv[2 * i + 1]});
}
