// The per-surfel rules of the body maps (staticfusion_amd/csrc/sf_body_map_rules.h) on the host, under the address and
// undefined-behaviour sanitizers: the pixel surfel, the move and the merge on hand cases -- a fronto-parallel plane under an
// identity camera, the depth gates met and missed, NaN and inf depths, a camera turned a quarter, every colour byte through the
// encoding, the weight cap, a normal that cancels --, on random cases against a plain fp64 restatement, and with guard words
// behind every 12-float output, which the functions must leave alone. The device runs the same text. Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_body_map_rules.h"

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

struct Out {
    std::vector<float> s;  // 12 floats and a guard of 8 behind them
    Out() : s(20, -5.f) {}
    bool guard() const {
        for (int i = 12; i < 20; i++)
            if (s[(size_t)i] != -5.f) return false;
        return true;
    }
    bool untouched() const {
        for (int i = 0; i < 12; i++)
            if (s[(size_t)i] != -5.f) return false;
        return guard();
    }
};

static const float I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static const float NaN = std::numeric_limits<float>::quiet_NaN();
static const float Inf = std::numeric_limits<float>::infinity();

static bool surfel(const float *z5, int v, int u, const float *pose, float fx, float fy, Out &o, int r = 128, int g = 128, int b = 128, float z_max = 8.f,
                   float dz = 0.05f) {
    const bool has = sfp_pixel_surfel_core(z5, v, u, pose, 10.f, 8.f, fx, fy, r, g, b, z_max, dz, 0.1f, 7.f, o.s.data());
    CHECK(o.guard());
    if (!has) CHECK(o.untouched());
    return has;
}

int main() {
    // a fronto-parallel plane at 2 m under an identity camera: the normal is (0, 0, 1), away from the camera; X = P
    {
        const float z5[5] = {2.f, 2.f, 2.f, 2.f, 2.f};
        Out o;
        CHECK(surfel(z5, 8, 10, I4, 100.f, 100.f, o));
        CHECK(o.s[0] == 0.f && o.s[1] == 0.f && o.s[2] == 2.f && o.s[3] == 0.1f && o.s[5] == 1.f && o.s[6] == 7.f && o.s[7] == 7.f);
        CHECK(o.s[8] == 0.f && o.s[9] == 0.f && o.s[10] == 1.f);
        CHECK(o.s[4] == (float)((128 << 16) + (128 << 8) + 128));
        const float r0 = (2.f / 100.f) * 1.41421356237f;
        CHECK(o.s[11] == r0);  // |n.z| = 1: r0 / 1 < 2 r0
        Out p;
        CHECK(surfel(z5, 12, 20, I4, 100.f, 50.f, p));  // (v - cy) * z / fy = 4 * 2 / 50
        CHECK(p.s[0] == (10.f * 2.f) / 100.f && p.s[1] == (4.f * 2.f) / 50.f && p.s[11] == (2.f / 75.f) * 1.41421356237f);
    }
    // the gates: z_max met and missed, normal_dz met and one ulp beyond, zero and negative depths, NaN and inf anywhere
    {
        Out o;
        const float at[5] = {8.f, 8.f, 8.f, 8.f, 8.f};
        CHECK(surfel(at, 5, 5, I4, 100.f, 100.f, o));
        for (int k = 0; k < 5; k++) {
            for (float bad : {std::nextafterf(8.f, 9.f), 0.f, -1.f, NaN, Inf, -Inf}) {
                float z5[5] = {8.f, 8.f, 8.f, 8.f, 8.f};
                z5[k] = bad;
                Out q;
                CHECK(!surfel(z5, 5, 5, I4, 100.f, 100.f, q));
            }
        }
        const float dz = 0.05f;
        for (int k = 1; k < 5; k++) {
            float z5[5] = {2.f, 2.f, 2.f, 2.f, 2.f};
            z5[k] = 2.f + dz;
            const bool met = std::fabs(z5[k] - 2.f) <= dz;  // (the sum is rounded: ask the same question)
            Out q;
            CHECK(surfel(z5, 5, 5, I4, 100.f, 100.f, q) == met);
            z5[k] = std::nextafterf(2.f + 2.f * dz, 9.f);
            Out r;
            CHECK(!surfel(z5, 5, 5, I4, 100.f, 100.f, r));
        }
        // exactly met in both directions with a power of two
        const float zs[5] = {2.f, 2.25f, 1.75f, 2.25f, 1.75f};
        Out q;
        CHECK(surfel(zs, 5, 5, I4, 100.f, 100.f, q, 1, 2, 3, 8.f, 0.25f));
        const float zb[5] = {2.f, std::nextafterf(2.25f, 3.f), 1.75f, 2.25f, 1.75f};
        Out r;
        CHECK(!surfel(zb, 5, 5, I4, 100.f, 100.f, r, 1, 2, 3, 8.f, 0.25f));
    }
    // a camera turned a quarter about y, shifted: X = R P + t and N = R n, with exact entries
    {
        const float pose[16] = {0, 0, -1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0.5f, -0.25f, 2.f, 1};  // x -> -z, z -> x
        const float z5[5] = {2.f, 2.f, 2.f, 2.f, 2.f};
        Out o;
        CHECK(surfel(z5, 8, 60, pose, 100.f, 100.f, o));
        CHECK(o.s[0] == 2.f + 0.5f && o.s[1] == -0.25f && o.s[2] == -1.f + 2.f);  // P = (1, 0, 2)
        CHECK(o.s[8] == 1.f && o.s[9] == 0.f && o.s[10] == 0.f);
    }
    // every colour byte survives the encoding and the decoding; out-of-range channels and codes give 0
    for (int b = 0; b < 256; b++) {
        CHECK(sfp_channel_byte((float)b / 255.0f) == b);
        float rgb[3];
        sfp_decode_colour(sfp_encode_colour((float)b / 255.0f, (float)(255 - b) / 255.0f, (float)((b * 7) & 255) / 255.0f), rgb);
        CHECK(rgb[0] == (float)b / 255.0f && rgb[1] == (float)(255 - b) / 255.0f && rgb[2] == (float)((b * 7) & 255) / 255.0f);
    }
    CHECK(sfp_channel_byte(NaN) == 0 && sfp_channel_byte(-1.f) == 0 && sfp_channel_byte(1.01f) == 0 && sfp_channel_byte(Inf) == 0 && sfp_channel_byte(3e38f) == 0);
    for (float c : {NaN, -1.f, 16777216.f, 3e9f, Inf, -Inf}) {
        float rgb[3];
        sfp_decode_colour(c, rgb);
        CHECK(rgb[0] == 0.f && rgb[1] == 0.f && rgb[2] == 0.f);
    }
    // the move: the identity leaves every bit, a translation moves the position alone
    {
        float s[12];
        for (int k = 0; k < 12; k++) s[k] = (float)uniform(-2, 2);
        Out o;
        sfp_move_core(I4, s, o.s.data());
        CHECK(o.guard());
        for (int k = 0; k < 12; k++) CHECK(o.s[(size_t)k] == s[k]);
        const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.5f, -1.f, 2.f, 1};
        Out p;
        sfp_move_core(T, s, p.s.data());
        CHECK(p.s[0] == s[0] + 0.5f && p.s[1] == s[1] - 1.f && p.s[2] == s[2] + 2.f && p.s[8] == s[8] && p.s[9] == s[9] && p.s[10] == s[10] && p.guard());
        float t[12];
        for (int k = 0; k < 12; k++) t[k] = s[k];
        sfp_move_core(T, t, t);  // in place
        for (int k = 0; k < 12; k++) CHECK(t[k] == p.s[(size_t)k]);
    }
    // the merge by hand: weight 1 averages, the confidence closes a quarter of its gap, the cap holds, a cancelling normal stays
    {
        const float s[12] = {1.f, 2.f, 3.f, 0.2f, (float)((10 << 16) + (20 << 8) + 30), 1.f, 3.f, 4.f, 0.f, 0.f, 1.f, 0.5f};
        const float p[12] = {2.f, 4.f, 5.f, 0.1f, (float)((20 << 16) + (40 << 8) + 50), 1.f, 9.f, 9.f, 0.f, 1.f, 0.f, 1.5f};
        Out o;
        sfp_merge_core(s, p, 0.25f, 32.f, 9.f, o.s.data());
        CHECK(o.guard());
        CHECK(o.s[0] == 1.5f && o.s[1] == 3.f && o.s[2] == 4.f && o.s[11] == 1.f && o.s[5] == 2.f && o.s[6] == 3.f && o.s[7] == 9.f);
        CHECK(o.s[3] == 0.2f + 0.25f * (1.0f - 0.2f));
        CHECK(o.s[4] == (float)((15 << 16) + (30 << 8) + 40));
        const float h = 0.5f / std::sqrt(0.5f);
        CHECK(o.s[8] == 0.f && o.s[9] == h && o.s[10] == h);
        float heavy[12];
        for (int k = 0; k < 12; k++) heavy[k] = s[k];
        heavy[5] = 1000.f;
        Out c;
        sfp_merge_core(heavy, p, 0.25f, 3.f, 9.f, c.s.data());  // w = 3: (3 * 1 + 2) / 4
        CHECK(c.s[0] == 1.25f && c.s[5] == 1001.f);
        heavy[5] = NaN;  // fminf gives the cap
        Out d;
        sfp_merge_core(heavy, p, 0.25f, 3.f, 9.f, d.s.data());
        CHECK(d.s[0] == 1.25f && d.s[5] != d.s[5]);
        float anti[12];
        for (int k = 0; k < 12; k++) anti[k] = p[k];
        anti[8] = 0.f; anti[9] = 0.f; anti[10] = -1.f;  // w = 1: the blend is the zero vector
        Out e;
        sfp_merge_core(s, anti, 0.25f, 32.f, 9.f, e.s.data());
        CHECK(e.s[8] == 0.f && e.s[9] == 0.f && e.s[10] == 1.f);
        float t[12];
        for (int k = 0; k < 12; k++) t[k] = s[k];
        sfp_merge_core(t, p, 0.25f, 32.f, 9.f, t);  // in place
        for (int k = 0; k < 12; k++) CHECK(t[k] == o.s[(size_t)k]);
    }
    // random pixels against a plain fp64 restatement of the geometry
    int with_normal = 0;
    for (int it = 0; it < 3000; it++) {
        const double fx = uniform(50, 300), fy = uniform(50, 300);
        const int v = (int)uniform(1, 200), u = (int)uniform(1, 300);
        const double z = uniform(0.3, 7.0);
        float z5[5];
        z5[0] = (float)z;
        for (int k = 1; k < 5; k++) z5[k] = (float)(z + uniform(-0.06, 0.06));
        float pose[16];
        const double ang = uniform(-3, 3);
        const float rot[16] = {(float)std::cos(ang), (float)std::sin(ang), 0, 0, (float)-std::sin(ang), (float)std::cos(ang), 0, 0, 0, 0, 1, 0,
                               (float)uniform(-2, 2), (float)uniform(-2, 2), (float)uniform(-2, 2), 1};
        for (int k = 0; k < 16; k++) pose[k] = rot[k];
        Out o;
        const bool has = sfp_pixel_surfel_core(z5, v, u, pose, 10.f, 8.f, (float)fx, (float)fy, 1, 2, 3, 8.f, 0.05f, 0.1f, 3.f, o.s.data());
        CHECK(o.guard());
        bool want = true;
        for (int k = 1; k < 5; k++) want = want && std::fabs(z5[k] - z5[0]) <= 0.05f;
        CHECK(has == want);
        if (!has) continue;
        with_normal++;
        auto bp = [&](int vv, int uu, double zz, double *P) {
            P[0] = ((double)uu - 10.0) * zz / (double)(float)fx;
            P[1] = ((double)vv - 8.0) * zz / (double)(float)fy;
            P[2] = zz;
        };
        double pl[3], prr[3], pu[3], pd[3], pc[3];
        bp(v, u - 1, z5[1], pl); bp(v, u + 1, z5[2], prr); bp(v - 1, u, z5[3], pu); bp(v + 1, u, z5[4], pd); bp(v, u, z5[0], pc);
        const double a[3] = {prr[0] - pl[0], prr[1] - pl[1], prr[2] - pl[2]}, b[3] = {pd[0] - pu[0], pd[1] - pu[1], pd[2] - pu[2]};
        double c[3] = {a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]};
        const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int k = 0; k < 3; k++) c[k] /= len;
        for (int r = 0; r < 3; r++) {
            const double X = pose[r] * pc[0] + pose[4 + r] * pc[1] + pose[8 + r] * pc[2] + pose[12 + r];
            const double N = pose[r] * c[0] + pose[4 + r] * c[1] + pose[8 + r] * c[2];
            CHECK(std::fabs(o.s[(size_t)r] - X) < 1e-4);
            CHECK(std::fabs(o.s[(size_t)(8 + r)] - N) < 2e-3);  // (the cross product of two short float differences)
        }
        const double r0 = z5[0] / (((double)(float)fx + (double)(float)fy) / 2.0) * 1.41421356237;
        CHECK(std::fabs(o.s[11] - std::fmin(2.0 * r0, r0 / std::fabs(c[2]))) < 1e-3 * r0 + 1e-7);
        double away = 0.0;  // N . (X - t) = n . P: the normal points away from the camera, whatever the depth steps are
        for (int r = 0; r < 3; r++) away += (double)o.s[(size_t)(8 + r)] * ((double)o.s[(size_t)r] - (double)pose[12 + r]);
        CHECK(away > 0.0 && c[0] * pc[0] + c[1] * pc[1] + c[2] * pc[2] > 0.0);
        // a merge of the surfel into a random neighbour: a convex combination, weight by weight
        float s[12];
        for (int k = 0; k < 12; k++) s[k] = o.s[(size_t)k] + (float)uniform(-0.01, 0.01);
        s[3] = (float)uniform(0, 1);
        s[4] = o.s[4];
        s[5] = (float)(int)uniform(1, 50);
        Out m;
        sfp_merge_core(s, o.s.data(), 0.25f, 32.f, 4.f, m.s.data());
        CHECK(m.guard());
        const double w = std::fmin((double)s[5], 32.0);
        for (int k = 0; k < 3; k++) CHECK(std::fabs(m.s[(size_t)k] - (w * s[k] + o.s[(size_t)k]) / (w + 1.0)) < 1e-5);
        const double nl = std::sqrt((double)m.s[8] * m.s[8] + (double)m.s[9] * m.s[9] + (double)m.s[10] * m.s[10]);
        CHECK(std::fabs(nl - 1.0) < 1e-5 && m.s[3] >= s[3] && m.s[3] <= 1.f && m.s[5] == s[5] + 1.f && m.s[7] == 4.f && m.s[6] == s[6] && m.s[4] == s[4]);
    }
    CHECK(with_normal > 500);
    if (failures) return 1;
    std::printf("ok %lld\n", checked);
    return 0;
}
