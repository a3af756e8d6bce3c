// sf_deform_solve.h — the SOLVE of include/sf_deform.h: rigid transforms of the nodes of a deformation graph from point
// constraints, by Gauss-Newton on dense normal equations. Host only. fp64 in the written order, only + - * / (no
// contraction: -ffp-contract=off); the bindings and the edges are those of sf_deform_rules.h, in fp32. sfd_solve of
// sf_hip_deform.hip checks its arguments and calls sfd_solve_core; tests/deform_ref.py restates it bit for bit. It includes
// nothing of the library but the rules.
#pragma once
#include <vector>

#include "sf_deform_rules.h"

#define SFD_SOLVE_OK 0
#define SFD_SOLVE_DEGENERATE 2
#define SFD_SOLVE_MAX_NODES 256
#define SFD_SOLVE_MAX_ITERATIONS 32

struct SfdConstraint {  // struct sfd_constraint of include/sf_deform.h
    float src[3], dst[3], time, weight;
};

struct SfdSolveState {
    int G = 0, n = 0;                // nodes; 6 G unknowns
    std::vector<double> R, t, g;     // per node: 9 (row-major), 3, 3
    std::vector<double> H, b;        // n x n (row-major), n
    std::vector<int> edges;          // 4 per node, -1: none
    std::vector<int> bind_m, bind_idx;  // per constraint: m, 4 indices
    std::vector<double> bind_w;      // per constraint: 4 weights
    int n_bound = 0, n_edges = 0;
};

// K = -[q]x, so that (Cayley(w) q - q) is K w to first order
static inline void sfd_neg_cross(const double *q, double K[3][3]) {
    K[0][0] = 0.0;   K[0][1] = q[2];  K[0][2] = -q[1];
    K[1][0] = -q[2]; K[1][1] = 0.0;   K[1][2] = q[0];
    K[2][0] = q[1];  K[2][1] = -q[0]; K[2][2] = 0.0;
}

// q = R d
static inline void sfd_rotate(const double *R, const double *d, double *q) {
    for (int r = 0; r < 3; r++) q[r] = (R[3 * r] * d[0] + R[3 * r + 1] * d[1]) + R[3 * r + 2] * d[2];
}

// One residual vector res[3] with weight wgt and Jacobian J (3 rows, 6 columns per listed node) into the energy and, with
// accumulate, into H and b: rows in order, and per row H[a][c] += wgt * (J[a] * J[c]), b[a] += wgt * (J[a] * res).
static inline void sfd_add_residual(SfdSolveState &s, bool accumulate, double wgt, const double *res, int n_nodes, const int *nodes, const double (*J)[24], double *energy) {
    *energy = *energy + wgt * ((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]);
    if (!accumulate) return;
    const int cols = 6 * n_nodes;
    for (int r = 0; r < 3; r++)
        for (int a = 0; a < cols; a++) {
            const size_t ga = (size_t)6 * nodes[a / 6] + a % 6;
            for (int c = 0; c < cols; c++) {
                const size_t gc = (size_t)6 * nodes[c / 6] + c % 6;
                s.H[ga * s.n + gc] = s.H[ga * s.n + gc] + wgt * (J[r][a] * J[r][c]);
            }
            s.b[ga] = s.b[ga] + wgt * (J[r][a] * res[r]);
        }
}

// The energy at the state's transforms; with accumulate, H and b (cleared first) as well. Constraints in index order, then
// the edges by (j, slot).
static inline double sfd_energy(SfdSolveState &s, bool accumulate, int C, const SfdConstraint *cons, double w_reg) {
    if (accumulate) {
        std::fill(s.H.begin(), s.H.end(), 0.0);
        std::fill(s.b.begin(), s.b.end(), 0.0);
    }
    double energy = 0.0;
    double J[3][24];
    for (int c = 0; c < C; c++) {
        const int m = s.bind_m[(size_t)c];
        if (m == 0) continue;
        const int *idx = &s.bind_idx[(size_t)4 * c];
        const double *wn = &s.bind_w[(size_t)4 * c];
        double v[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < m; i++) {
            const int j = idx[i];
            const double *g = &s.g[(size_t)3 * j], *R = &s.R[(size_t)9 * j], *t = &s.t[(size_t)3 * j];
            const double d[3] = {(double)cons[c].src[0] - g[0], (double)cons[c].src[1] - g[1], (double)cons[c].src[2] - g[2]};
            double q[3], K[3][3];
            sfd_rotate(R, d, q);
            sfd_neg_cross(q, K);
            for (int r = 0; r < 3; r++) {
                const double phi = (q[r] + g[r]) + t[r];
                const double term = wn[i] * phi;
                v[r] = i == 0 ? term : v[r] + term;
                for (int k = 0; k < 3; k++) {
                    J[r][6 * i + k] = wn[i] * K[r][k];
                    J[r][6 * i + 3 + k] = wn[i] * (r == k ? 1.0 : 0.0);
                }
            }
        }
        const double res[3] = {v[0] - (double)cons[c].dst[0], v[1] - (double)cons[c].dst[1], v[2] - (double)cons[c].dst[2]};
        sfd_add_residual(s, accumulate, (double)cons[c].weight, res, m, idx, J, &energy);
    }
    for (int j = 0; j < s.G; j++)
        for (int slot = 0; slot < 4; slot++) {
            const int k = s.edges[(size_t)4 * j + slot];
            if (k < 0) continue;
            const double *gj = &s.g[(size_t)3 * j], *gk = &s.g[(size_t)3 * k];
            const double d[3] = {gk[0] - gj[0], gk[1] - gj[1], gk[2] - gj[2]};
            double q[3], K[3][3], res[3];
            sfd_rotate(&s.R[(size_t)9 * j], d, q);
            sfd_neg_cross(q, K);
            for (int r = 0; r < 3; r++) {
                res[r] = (((q[r] + gj[r]) + s.t[(size_t)3 * j + r]) - gk[r]) - s.t[(size_t)3 * k + r];
                for (int c = 0; c < 3; c++) {
                    J[r][c] = K[r][c];
                    J[r][3 + c] = r == c ? 1.0 : 0.0;
                    J[r][6 + c] = 0.0;
                    J[r][9 + c] = r == c ? -1.0 : 0.0;
                }
            }
            const int nodes[2] = {j, k};
            sfd_add_residual(s, accumulate, w_reg, res, 2, nodes, J, &energy);
        }
    return energy;
}

// (H + damping I) x = -b by LDL^T without pivoting, in place in H (right-looking: pivot k is subtracted from what lies
// behind it, so every element loses the same terms in the same order as in the row-wise form of the alignment step). A pivot
// that is not > floor_d: false.
static inline bool sfd_ldlt_solve(SfdSolveState &s, double damping, double floor_d, std::vector<double> &x) {
    const size_t n = (size_t)s.n;
    double *A = s.H.data();
    for (size_t k = 0; k < n; k++) A[k * n + k] = A[k * n + k] + damping;
    std::vector<double> col(n);
    for (size_t k = 0; k < n; k++) {
        const double dk = A[k * n + k];
        if (!(dk > floor_d)) return false;
        for (size_t i = k + 1; i < n; i++) col[i] = A[i * n + k] / dk;
        for (size_t i = k + 1; i < n; i++) {
            const double li = col[i];
            double *row = A + i * n;
            for (size_t j = k + 1; j <= i; j++) row[j] = row[j] - (li * col[j]) * dk;
        }
        for (size_t i = k + 1; i < n; i++) A[i * n + k] = col[i];  // L below the diagonal, d on it
    }
    x.assign(n, 0.0);
    std::vector<double> z(n);
    for (size_t i = 0; i < n; i++) {
        double v = -s.b[i];
        for (size_t k = 0; k < i; k++) v = v - A[i * n + k] * z[k];
        z[i] = v;
    }
    for (size_t i = n; i-- > 0;) {
        double v = z[i] / A[i * n + i];
        for (size_t k = i + 1; k < n; k++) v = v - A[k * n + i] * x[k];
        x[i] = v;
    }
    return true;
}

// R <- Cayley(w) R and t <- t + u for every node (the Cayley map of the alignment step)
static inline void sfd_update(SfdSolveState &s, const std::vector<double> &x) {
    for (int j = 0; j < s.G; j++) {
        const double *xj = &x[(size_t)6 * j];
        const double a0 = 0.5 * xj[0], a1 = 0.5 * xj[1], a2 = 0.5 * xj[2];
        const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
        const double sc = 2.0 / (1.0 + aa);
        double Q[3][3];
        Q[0][0] = 1.0 - sc * (a1 * a1 + a2 * a2);
        Q[0][1] = sc * (a0 * a1 - a2);
        Q[0][2] = sc * (a0 * a2 + a1);
        Q[1][0] = sc * (a0 * a1 + a2);
        Q[1][1] = 1.0 - sc * (a0 * a0 + a2 * a2);
        Q[1][2] = sc * (a1 * a2 - a0);
        Q[2][0] = sc * (a0 * a2 - a1);
        Q[2][1] = sc * (a1 * a2 + a0);
        Q[2][2] = 1.0 - sc * (a0 * a0 + a1 * a1);
        double *R = &s.R[(size_t)9 * j];
        double out[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) out[3 * r + c] = (Q[r][0] * R[c] + Q[r][1] * R[3 + c]) + Q[r][2] * R[6 + c];
        for (int k = 0; k < 9; k++) R[k] = out[k];
        for (int r = 0; r < 3; r++) s.t[(size_t)3 * j + r] = s.t[(size_t)3 * j + r] + xj[3 + r];
    }
}

// energies: iterations + 1 doubles (the energy before every iteration done and after the last; the rest 0). Returns the
// status; *done the iterations done; M (12 floats per node, row-major [R | t]) is rewritten from the state the last
// completed iteration left.
static inline int sfd_solve_core(int G, const float *pos, const float *times, int C, const SfdConstraint *cons, float time_window, float w_reg, float damping,
                                 int iterations, float *M, int *done, int *n_bound, double *energies) {
    SfdSolveState s;
    s.G = G;
    s.n = 6 * G;
    s.R.resize((size_t)9 * G);
    s.t.resize((size_t)3 * G);
    s.g.resize((size_t)3 * G);
    s.H.resize((size_t)s.n * s.n);
    s.b.resize((size_t)s.n);
    s.edges.resize((size_t)4 * G);
    s.bind_m.assign((size_t)C, 0);
    s.bind_idx.assign((size_t)4 * C, -1);
    s.bind_w.assign((size_t)4 * C, 0.0);
    for (int j = 0; j < G; j++) {
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) s.R[(size_t)9 * j + 3 * r + c] = (double)M[(size_t)12 * j + 4 * r + c];
            s.t[(size_t)3 * j + r] = (double)M[(size_t)12 * j + 4 * r + 3];
            s.g[(size_t)3 * j + r] = (double)pos[(size_t)3 * j + r];
        }
        sfd_edges_core(G, pos, times, time_window, j, &s.edges[(size_t)4 * j]);
        for (int k = 0; k < 4; k++) s.n_edges += s.edges[(size_t)4 * j + k] >= 0;
    }
    for (int c = 0; c < C; c++) {
        float w[4];
        const int m = sfd_bind_core(G, pos, times, time_window, cons[c].src, cons[c].time, -1, &s.bind_idx[(size_t)4 * c], w);
        s.bind_m[(size_t)c] = m;
        for (int k = 0; k < 4; k++) s.bind_w[(size_t)4 * c + k] = (double)w[k];
        s.n_bound += m > 0;
    }
    *n_bound = s.n_bound;
    const double floor_d = 1e-9 * (double)(s.n_bound + s.n_edges);
    int status = SFD_SOLVE_OK, it = 0;
    std::vector<double> x;
    for (; it < iterations; it++) {
        energies[it] = sfd_energy(s, true, C, cons, (double)w_reg);
        if (!sfd_ldlt_solve(s, (double)damping, floor_d, x)) {
            status = SFD_SOLVE_DEGENERATE;
            break;
        }
        sfd_update(s, x);
    }
    if (status == SFD_SOLVE_OK) energies[it] = sfd_energy(s, false, C, cons, (double)w_reg);
    *done = it;
    for (int j = 0; j < G; j++)
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) M[(size_t)12 * j + 4 * r + c] = (float)s.R[(size_t)9 * j + 3 * r + c];
            M[(size_t)12 * j + 4 * r + 3] = (float)s.t[(size_t)3 * j + r];
        }
    return status;
}
