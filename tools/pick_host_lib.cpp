// csrc/pick.h behind the two entry points' argument lists, on host memory: what the kernels of csrc/pick.hip compute, row by row and
// camera by camera, for the tests without a GPU (tests/test_pick_cpu.py builds it as a shared library with the system compiler and
// lets the recording stand-in of tests/pick_fake.py answer through it).  Plain C++, no HIP, no argument checks:
//   c++ -std=c++17 -O1 -shared -fPIC -I sparf_amd/csrc tools/pick_host_lib.cpp -o libpick_host.so
#include "pick.h"

using namespace sparf;

extern "C" int host_pick_pixels(const int64_t* perm_a, int n_a, const int64_t* perm_b, int n_b, int a_w, int a_h, int b_x0, int b_y0, int b_w, int b_h,
                                int W, int patch, float* pixels, int64_t* rays) {
    PickPixelsArgs a{};
    a.perm_a = perm_a; a.perm_b = perm_b; a.n_a = n_a; a.n_b = n_b; a.a_w = a_w; a.a_h = a_h;
    a.b_x0 = b_x0; a.b_y0 = b_y0; a.b_w = b_w; a.b_h = b_h; a.W = W; a.patch = patch; a.rows = (n_a + n_b) * patch * patch;
    a.pixels = pixels; a.rays = rays;
    for (int r = 0; r < a.rows; ++r) pick_row(a, r);
    return 0;
}

extern "C" int host_unseen_pose(const float* poses_w2c, int row_floats, int B, int id_self, float w, float one_minus_w, float* pose_w2c_ref,
                                float* pose_c2w_ref, float* pose_c2w_other, float* pose_w2c_at_unseen, int32_t* id_other) {
    UnseenPoseArgs a{};
    a.poses_w2c = poses_w2c; a.row_floats = row_floats; a.B = B; a.id_self = id_self; a.w = w; a.one_minus_w = one_minus_w;
    a.w2c_ref = pose_w2c_ref; a.c2w_ref = pose_c2w_ref; a.c2w_other = pose_c2w_other; a.w2c_unseen = pose_w2c_at_unseen; a.id_other = id_other;
    double best;
    int at;
    pick_nearest(a, 0, 1, best, at);
    for (int e = 0; e < 16; ++e) pick_pose_outputs(a, at, e);
    id_other[0] = (int32_t)at;
    return 0;
}
