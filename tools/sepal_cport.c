/* CPU baseline of sq.gr.sepal: a C port of the reference's `_diffusion` (gr/_sepal.py:208-254) for one gene, the loop numba
 * compiles per gene, and an OpenMP loop over genes (the reference's thread_map, one gene per thread).  Built and timed by
 * tools/sepal_time.py; float64 throughout, the neighbour sum left to right, the entropy of `_entropy` (:290-305). */
#include <math.h>
#include <omp.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static double entropy(const double* c, const int32_t* sat, int64_t n_sat) {
    const double eps = 2.220446049250313e-16;
    double s = 0.0;
    for (int64_t j = 0; j < n_sat; ++j)
        if (c[sat[j]] > 0) s += c[sat[j]];
    if (s < eps) return 0.0;
    double h = 0.0;
    for (int64_t j = 0; j < n_sat; ++j) {
        const double v = c[sat[j]];
        if (v > 0) {
            const double x = v / s;
            h += -log(x < eps ? eps : x) * x;
        }
    }
    return h;
}

/* returns the stop sweep or -1 */
int32_t sepal_diffusion(double* conc, int64_t n, int use_hex, int32_t n_iter, const int32_t* sat, int64_t n_sat, const int32_t* sat_idx,
                        int32_t K, const int32_t* unsat, int64_t n_unsat, const int32_t* nearest, double dt, double thresh) {
    double* dcdt = (double*)calloc((size_t)n, sizeof(double));
    double prev = 1.0;
    int32_t stop = -1;
    for (int32_t i = 0; i < n_iter; ++i) {
        for (int64_t j = 0; j < n_sat; ++j) {
            double s = conc[sat_idx[j * K]];
            for (int k = 1; k < K; ++k) s = s + conc[sat_idx[j * K + k]];
            const double c = conc[sat[j]];
            dcdt[sat[j]] = use_hex ? (2.0 * s - 12.0 * c) / 3.0 : s - 4.0 * c;
        }
        for (int64_t j = 0; j < n_sat; ++j) conc[sat[j]] += dcdt[sat[j]] * dt;
        for (int64_t q = 0; q < n_unsat; ++q) conc[unsat[q]] += dcdt[nearest[q]] * dt;
        for (int64_t j = 0; j < n; ++j)
            if (conc[j] < 0) conc[j] = 0;
        const double ent = entropy(conc, sat, n_sat) / (double)n_sat;
        const double d = fabs(ent - prev);
        prev = ent;
        if (d <= thresh) {
            stop = i;
            break;
        }
    }
    free(dcdt);
    return stop;
}

/* genes: X gene-major [G][n] (overwritten); out[g] = stop sweep */
void sepal_genes(double* X, int64_t G, int64_t n, int use_hex, int32_t n_iter, const int32_t* sat, int64_t n_sat, const int32_t* sat_idx,
                 int32_t K, const int32_t* unsat, int64_t n_unsat, const int32_t* nearest, double dt, double thresh, int32_t* out) {
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t g = 0; g < G; ++g)
        out[g] = sepal_diffusion(X + g * n, n, use_hex, n_iter, sat, n_sat, sat_idx, K, unsat, n_unsat, nearest, dt, thresh);
}

void sepal_set_threads(int n) { omp_set_num_threads(n); }
