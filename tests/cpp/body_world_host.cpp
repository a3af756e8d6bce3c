// The world motion of the region motions (staticfusion_amd/csrc/sf_body_world.h) on the host, under the address and
// undefined-behaviour sanitizers: W = (T1 * D) * T0^-1 on hand cases -- identity, a region that did not move under a camera
// that moved, a pure translation, a quarter turn about each axis, the inverse of a motion composed with it --, on 2000 random
// rigid triples against a plain fp64 matrix product, and with guards behind both 16-float outputs, which the functions must
// leave alone. The device runs the same text. Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_body_world.h"

static long long checked = 0;
static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        checked++;                                                    \
        if (!(cond)) {                                                \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);       \
            failures++;                                               \
        }                                                             \
    } while (0)

static uint64_t state = 88172645463325252ull;
static double uniform(double lo, double hi) {
    state = 6364136223846793005ull * state + 1442695040888963407ull;
    return lo + (hi - lo) * (double)(state >> 11) / 9007199254740992.0;
}

struct M4 {
    double m[4][4];
};
static M4 identity() {
    M4 r{};
    for (int i = 0; i < 4; i++) r.m[i][i] = 1.0;
    return r;
}
static M4 mul(const M4 &a, const M4 &b) {
    M4 r{};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 4; k++) r.m[i][j] += a.m[i][k] * b.m[k][j];
    return r;
}
static M4 rigid_inverse(const M4 &a) {
    M4 r = identity();
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[j][i];
    for (int i = 0; i < 3; i++) r.m[i][3] = -(r.m[i][0] * a.m[0][3] + r.m[i][1] * a.m[1][3] + r.m[i][2] * a.m[2][3]);
    return r;
}
static M4 turn(int axis, double angle, double tx, double ty, double tz) {
    M4 r = identity();
    const int a = (axis + 1) % 3, b = (axis + 2) % 3;
    r.m[a][a] = std::cos(angle);
    r.m[a][b] = -std::sin(angle);
    r.m[b][a] = std::sin(angle);
    r.m[b][b] = std::cos(angle);
    r.m[0][3] = tx;
    r.m[1][3] = ty;
    r.m[2][3] = tz;
    return r;
}
static M4 random_rigid() {
    M4 r = identity();
    for (int axis = 0; axis < 3; axis++) r = mul(r, turn(axis, uniform(-3.0, 3.0), 0, 0, 0));
    for (int i = 0; i < 3; i++) r.m[i][3] = uniform(-5.0, 5.0);
    return r;
}
// a pose as the library takes it: column-major floats; and the matrix those floats stand for
static void as_pose(const M4 &a, float *p) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) p[r + 4 * c] = (float)a.m[r][c];
}
static M4 of_pose(const float *p) {
    M4 a{};
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) a.m[r][c] = (double)p[r + 4 * c];
    return a;
}

struct Out {
    std::vector<float> w;  // 16 floats and a guard of 8 behind them
    Out() : w(24, -5.f) {}
    bool guard() const {
        for (int i = 16; i < 24; i++)
            if (w[(size_t)i] != -5.f) return false;
        return true;
    }
};

static Out world(const float *p0, const float *p1, const M4 &D) {
    std::vector<double> d(12);
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) d[(size_t)(4 * k + c)] = D.m[k][c];
    Out o;
    sfb_world_core(p0, p1, d.data(), o.w.data());
    CHECK(o.guard());
    CHECK(o.w[3] == 0.f && o.w[7] == 0.f && o.w[11] == 0.f && o.w[15] == 1.f);
    Out e;
    sfb_estimate_as_4x4(d.data(), e.w.data());
    CHECK(e.guard() && e.w[3] == 0.f && e.w[7] == 0.f && e.w[11] == 0.f && e.w[15] == 1.f);
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) CHECK(e.w[(size_t)(k + 4 * c)] == (float)D.m[k][c]);
    return o;
}

static double distance(const Out &o, const M4 &want) {
    double worst = 0.0;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) worst = std::fmax(worst, std::fabs((double)o.w[(size_t)(r + 4 * c)] - want.m[r][c]));
    return worst;
}

int main() {
    float I[16], p0[16], p1[16];
    as_pose(identity(), I);
    // identity everywhere: exactly the identity
    {
        const Out o = world(I, I, identity());
        for (int i = 0; i < 16; i++) CHECK(o.w[(size_t)i] == (i % 5 == 0 ? 1.f : 0.f));
    }
    // a pure translation of the body under a camera at rest: W is that translation, exactly (small integers over powers of two)
    {
        const Out o = world(I, I, turn(0, 0.0, 0.25, -0.5, 2.0));
        CHECK(o.w[12] == 0.25f && o.w[13] == -0.5f && o.w[14] == 2.0f && o.w[0] == 1.f && o.w[5] == 1.f && o.w[10] == 1.f && o.w[4] == 0.f);
    }
    // a region that did not move under a camera that moved: D = T1^-1 T0 gives W = I to the rounding of the poses
    for (int axis = 0; axis < 3; axis++) {
        as_pose(turn(axis, 0.3, 0.1, -0.2, 0.3), p0);
        as_pose(turn((axis + 1) % 3, -0.2, -0.3, 0.2, 0.1), p1);
        const M4 D = mul(rigid_inverse(of_pose(p1)), of_pose(p0));
        CHECK(distance(world(p0, p1, D), identity()) < 1e-6);
    }
    // a quarter turn about each axis seen from an identity camera is that turn
    for (int axis = 0; axis < 3; axis++) {
        const M4 Q = turn(axis, 1.5707963267948966, 0.5, 0.25, -1.0);
        CHECK(distance(world(I, I, Q), Q) < 1e-7);
    }
    // random rigid triples: the written order against a plain product with the transpose inverse
    for (int it = 0; it < 2000; it++) {
        as_pose(random_rigid(), p0);
        as_pose(random_rigid(), p1);
        const M4 D = random_rigid();
        const M4 want = mul(mul(of_pose(p1), D), rigid_inverse(of_pose(p0)));
        CHECK(distance(world(p0, p1, D), want) < 1e-4);  // (entries up to ~ 100: a float rounding of them, far below this)
    }
    if (failures) return 1;
    std::printf("ok %lld\n", checked);
    return 0;
}
