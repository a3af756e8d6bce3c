// sf_deform_rules.h — the rules of include/sf_deform.h that the host and the device share: the BIND of a point to the nodes of a
// deformation graph (the best five by (d2, j), kept by ordered insertion; the weights), the DEFORM of a surfel under its
// binding, the EDGES of a node and the deformation of a pose. Plain C++, fp32 in the written order, one operation per
// expression (no contraction: -ffp-contract=off), so the host (the pure-host calls of sf_hip_deform.hip, and
// tests/cpp/deform_rules_host.cpp under the sanitizers) and the device (sf_deform.h) run the same text and give the same
// bits. It includes nothing of the library and defines no kernel.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFD_HD __host__ __device__
#else
#define SFD_HD
#endif

// The best five eligible nodes seen so far, ascending by (d2, j). A free place holds d2 = INFINITY and j = -1; an eligible
// node has d2 < INFINITY, so the strict comparison below fills free places and orders real ones alike.
struct SfdBest {
    float d2[5];
    int j[5];
};

SFD_HD static inline void sfd_best_init(SfdBest *b) {
    for (int k = 0; k < 5; k++) {
        b->d2[k] = INFINITY;
        b->j[k] = -1;
    }
}

// Node j at (gx, gy, gz) with time gt is offered to the point p with time tau. Nodes are offered in ascending j, so a node
// that ties with one already held goes behind it: the insertion moves past a held node only when d2 is strictly smaller.
SFD_HD static inline void sfd_best_offer(SfdBest *b, float gx, float gy, float gz, float gt, int j, const float *p, float tau, float time_window) {
    const float dx = p[0] - gx;
    const float dy = p[1] - gy;
    const float dz = p[2] - gz;
    const float xx = dx * dx;
    const float yy = dy * dy;
    const float zz = dz * dz;
    const float xy = xx + yy;
    const float d2 = xy + zz;
    const float dt = gt - tau;
    if (!(d2 < INFINITY && fabsf(dt) <= time_window)) return;
    if (!(d2 < b->d2[4])) return;
    b->d2[4] = d2;
    b->j[4] = j;
    // (four steps, no early exit: once a step does not swap, the places before it are in order and no later step swaps; with
    // constant indices the ten values stay in registers on the device)
    for (int k = 4; k > 0; k--) {
        const bool swap = b->d2[k] < b->d2[k - 1];
        const float lo_d = swap ? b->d2[k] : b->d2[k - 1], hi_d = swap ? b->d2[k - 1] : b->d2[k];
        const int lo_j = swap ? b->j[k] : b->j[k - 1], hi_j = swap ? b->j[k - 1] : b->j[k];
        b->d2[k - 1] = lo_d;
        b->j[k - 1] = lo_j;
        b->d2[k] = hi_d;
        b->j[k] = hi_j;
    }
}

// The binding from the best five: the number m of nodes taken (0: UNBOUND), their indices (a missing one -1) and weights (a
// missing one 0).
SFD_HD static inline int sfd_best_finish(const SfdBest *b, int *idx, float *w) {
    int m = 0;
    float last = 0.0f;  // the d2 of the m-th node
    for (int k = 0; k < 4; k++) {
        idx[k] = b->j[k];
        w[k] = 0.0f;
        if (b->j[k] >= 0) {
            m = k + 1;
            last = b->d2[k];
        }
    }
    if (m == 0) return 0;
    const float dmax2 = b->j[4] >= 0 ? b->d2[4] : 4.0f * last;
    if (dmax2 == 0.0f) {
        for (int k = 0; k < 4; k++)
            if (k < m) w[k] = 1.0f;
    } else {
        const float smax = sqrtf(dmax2);
        for (int k = 0; k < 4; k++)
            if (k < m) {
                const float s = sqrtf(b->d2[k]);
                const float ratio = s / smax;
                const float one_less = 1.0f - ratio;
                w[k] = one_less * one_less;
            }
    }
    float S = w[0];
    for (int k = 1; k < 4; k++)
        if (k < m) S = S + w[k];
    if (!(S > 0.0f)) {
        for (int k = 0; k < 4; k++)
            if (k < m) w[k] = 1.0f;
        S = (float)m;
    }
    for (int k = 0; k < 4; k++)
        if (k < m) w[k] = w[k] / S;
    return m;
}

// BIND of p with time tau over the G nodes (pos: 3 floats per node, times: one), node `skip` left out (-1: none).
SFD_HD static inline int sfd_bind_core(int G, const float *pos, const float *times, float time_window, const float *p, float tau, int skip, int *idx, float *w) {
    SfdBest b;
    sfd_best_init(&b);
    for (int j = 0; j < G; j++)
        if (j != skip) sfd_best_offer(&b, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], times[j], j, p, tau, time_window);
    return sfd_best_finish(&b, idx, w);
}

// (A v).r of a row-major 3 x 4 matrix M = [A | t]
SFD_HD static inline float sfd_rot_row(const float *M, int r, const float *v) {
    const float a = M[4 * r] * v[0];
    const float b = M[4 * r + 1] * v[1];
    const float c = M[4 * r + 2] * v[2];
    const float ab = a + b;
    return ab + c;
}

// phi(p).r = ((A d).r + g.r) + t.r with d = p - g
SFD_HD static inline float sfd_phi_row(const float *M, const float *g, int r, const float *d) {
    const float rot = sfd_rot_row(M, r, d);
    const float at_node = rot + g[r];
    return at_node + M[4 * r + 3];
}

// The blend of a position p and a direction n under a binding of m >= 1 nodes: g4 holds their positions (3 floats each), M4
// their transforms (12 floats each), w their weights. p_out: the ascending sum of w_i * phi_i(p); n_out: the ascending sum of
// w_i * (A_i n), not normalised. p_out may be p and n_out may be n.
SFD_HD static inline void sfd_blend_core(int m, const float *w, const float *g4, const float *M4, const float *p, const float *n, float *p_out, float *n_out) {
    float P[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 4; i++) {  // (a constant trip count: the device keeps g4 and M4 in registers)
        if (i >= m) continue;
        const float *g = g4 + 3 * i;
        const float *M = M4 + 12 * i;
        const float d[3] = {p[0] - g[0], p[1] - g[1], p[2] - g[2]};
        for (int r = 0; r < 3; r++) {
            const float a = w[i] * sfd_phi_row(M, g, r, d);
            const float b = w[i] * sfd_rot_row(M, r, n);
            P[r] = i == 0 ? a : P[r] + a;
            N[r] = i == 0 ? b : N[r] + b;
        }
    }
    for (int r = 0; r < 3; r++) {
        p_out[r] = P[r];
        n_out[r] = N[r];
    }
}

// DEFORM of the surfel s under a binding of m >= 1 nodes: position and normal change, s[3..7] and s[11] stay. out may be s.
SFD_HD static inline void sfd_deform_core(int m, const float *w, const float *g4, const float *M4, const float *s, float *out) {
    float P[3], N[3];
    sfd_blend_core(m, w, g4, M4, s, s + 8, P, N);
    const float xx = N[0] * N[0];
    const float yy = N[1] * N[1];
    const float zz = N[2] * N[2];
    const float xy = xx + yy;
    const float nn = xy + zz;
    for (int k = 3; k < 8; k++) out[k] = s[k];
    out[11] = s[11];
    if (nn > 0.0f && nn < INFINITY) {
        const float len = sqrtf(nn);
        for (int r = 0; r < 3; r++) out[8 + r] = N[r] / len;
    } else {
        for (int r = 0; r < 3; r++) out[8 + r] = s[8 + r];
    }
    for (int r = 0; r < 3; r++) out[r] = P[r];
}

// BIND and DEFORM of one surfel over host arrays (pos, times, M: 12 floats per node): m, and out written when m >= 1.
SFD_HD static inline int sfd_deform_surfel_core(int G, const float *pos, const float *times, const float *M, float time_window, const float *s, float *out) {
    int idx[4];
    float w[4], g4[12], M4[48];
    const int m = sfd_bind_core(G, pos, times, time_window, s, s[6], -1, idx, w);
    for (int i = 0; i < m; i++) {
        for (int k = 0; k < 3; k++) g4[3 * i + k] = pos[3 * idx[i] + k];
        for (int k = 0; k < 12; k++) M4[12 * i + k] = M[12 * (size_t)idx[i] + k];
    }
    if (m) sfd_deform_core(m, w, g4, M4, s, out);
    return m;
}

// EDGES of node j: the indices of BIND of g_j with tau = time_j over the other nodes
SFD_HD static inline void sfd_edges_core(int G, const float *pos, const float *times, float time_window, int j, int *edges4) {
    float w[4];
    sfd_bind_core(G, pos, times, time_window, pos + 3 * j, times[j], j, edges4, w);
}

SFD_HD static inline float sfd_dot3(const float *a, const float *b) {
    const float xx = a[0] * b[0];
    const float yy = a[1] * b[1];
    const float zz = a[2] * b[2];
    const float xy = xx + yy;
    return xy + zz;
}

// v / sqrtf(v . v): false (out untouched) unless 0 < v . v < INFINITY
SFD_HD static inline bool sfd_unit(const float *v, float *out) {
    const float vv = sfd_dot3(v, v);
    if (!(vv > 0.0f && vv < INFINITY)) return false;
    const float len = sqrtf(vv);
    for (int r = 0; r < 3; r++) out[r] = v[r] / len;
    return true;
}

// The pose (column-major 4 x 4) with time tau under the graph: the origin bound and deformed as a position, the three axes
// deformed as directions under the origin's binding and made orthonormal (include/sf_deform.h, POSE). Returns m; with
// m == 0 out is the pose as it was.
SFD_HD static inline int sfd_deform_pose_core(int G, const float *pos, const float *times, const float *M, float time_window, const float *pose, float tau, float *out) {
    int idx[4];
    float w[4], g4[12], M4[48];
    float o[16];
    for (int k = 0; k < 16; k++) o[k] = pose[k];
    const int m = sfd_bind_core(G, pos, times, time_window, pose + 12, tau, -1, idx, w);
    if (m) {
        for (int i = 0; i < m; i++) {
            for (int k = 0; k < 3; k++) g4[3 * i + k] = pos[3 * idx[i] + k];
            for (int k = 0; k < 12; k++) M4[12 * i + k] = M[12 * (size_t)idx[i] + k];
        }
        float P[3], a[3][3];
        for (int c = 0; c < 3; c++) sfd_blend_core(m, w, g4, M4, pose + 12, pose + 4 * c, P, a[c]);
        float x[3], y[3], z[3], yr[3], zr[3];
        bool ok = sfd_unit(a[0], x);
        if (ok) {
            const float xy = sfd_dot3(x, a[1]);
            for (int r = 0; r < 3; r++) {
                const float along = xy * x[r];
                yr[r] = a[1][r] - along;
            }
            ok = sfd_unit(yr, y);
        }
        if (ok) {
            const float xz = sfd_dot3(x, a[2]);
            const float yz = sfd_dot3(y, a[2]);
            for (int r = 0; r < 3; r++) {
                const float along_x = xz * x[r];
                const float along_y = yz * y[r];
                const float less_x = a[2][r] - along_x;
                zr[r] = less_x - along_y;
            }
            ok = sfd_unit(zr, z);
        }
        if (ok)
            for (int r = 0; r < 3; r++) {
                o[r] = x[r];
                o[4 + r] = y[r];
                o[8 + r] = z[r];
            }
        for (int r = 0; r < 3; r++) o[12 + r] = P[r];
    }
    for (int k = 0; k < 16; k++) out[k] = o[k];
    return m;
}
