// Rectangular linear sum assignment: the shortest-augmenting-path solver of scipy >= 1.4 (scipy.optimize.linear_sum_assignment),
// restated so that its result is scipy's, ties included.  Plain C++: compiled by the library's host entry point fnp_host_lsap
// and, as it stands, by the stand-alone sanitizer program tools/lsap_sanitize.cpp.  The device kernel of tfassign.hip walks the
// same steps with the scan of the remaining columns spread over a wave.
//
// What fixes the result beyond optimality, and so is part of this restatement:
//   * a matrix with fewer columns than rows is transposed first, so the solver's rows are the shorter side;
//   * the reduced cost is formed as ((minVal + cost) - u[i]) - v[j] in f64 on the f32 costs widened, in that order;
//   * `remaining` starts as nc-1 .. 0 and a column leaves it by a swap with the last entry: the scan order is that array's;
//   * the scan keeps the first position that attains the minimum, unless a later one attaining it is an unassigned column.
#pragma once
#include <limits>
#include <vector>

// cost: nr x nc row-major, nr <= nc (the caller transposes).  col4row (nr): the column of every row.  Returns false when no
// finite augmenting path exists (a NaN or an infinite cost: out of contract); every loop is bounded either way, because each
// inner step removes one column from `remaining`.
static inline bool fnp_lsap_solve(const std::vector<double> &cost, int nr, int nc, std::vector<int> &col4row) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u(nr, 0.0), v(nc, 0.0), spc(nc);
    std::vector<int> path(nc, -1), row4col(nc, -1), remaining(nc);
    std::vector<char> SR(nr), SC(nc);
    col4row.assign(nr, -1);
    for (int cur = 0; cur < nr; ++cur) {
        double min_val = 0.0;
        int nrem = nc, sink = -1, i = cur;
        for (int it = 0; it < nc; ++it) remaining[it] = nc - 1 - it;
        SR.assign(nr, 0), SC.assign(nc, 0), spc.assign(nc, inf);
        while (sink == -1) {
            int index = -1;
            double lowest = inf;
            SR[i] = 1;
            for (int it = 0; it < nrem; ++it) {
                const int j = remaining[it];
                const double r = ((min_val + cost[(size_t)i * nc + j]) - u[i]) - v[j];
                if (r < spc[j]) path[j] = i, spc[j] = r;
                if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) lowest = spc[j], index = it;
            }
            min_val = lowest;
            if (index < 0 || !(min_val < inf)) return false;
            const int j = remaining[index];
            if (row4col[j] == -1) sink = j;
            else i = row4col[j];
            SC[j] = 1;
            remaining[index] = remaining[--nrem];
        }
        u[cur] += min_val;
        for (int r = 0; r < nr; ++r)
            if (SR[r] && r != cur) u[r] += min_val - spc[col4row[r]];
        for (int j = 0; j < nc; ++j)
            if (SC[j]) v[j] -= min_val - spc[j];
        for (int j = sink;;) {
            const int r = path[j];
            row4col[j] = r;
            const int next = col4row[r];
            col4row[r] = j;
            j = next;
            if (r == cur) break;
        }
    }
    return true;
}

// scipy's call: cost nr x nc f32 row-major, any orientation -> min(nr, nc) pairs with `rows` ascending.
static inline bool fnp_lsap(const float *cost, int nr, int nc, int *rows, int *cols) {
    if (nr <= 0 || nc <= 0) return true;
    const bool transpose = nc < nr;
    const int sr = transpose ? nc : nr, sc = transpose ? nr : nc;
    std::vector<double> c((size_t)nr * nc);
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) {
            const double x = (double)cost[(size_t)i * nc + j];
            if (transpose) c[(size_t)j * nr + i] = x;
            else c[(size_t)i * nc + j] = x;
        }
    std::vector<int> col4row;
    if (!fnp_lsap_solve(c, sr, sc, col4row)) return false;
    if (!transpose) {
        for (int i = 0; i < nr; ++i) rows[i] = i, cols[i] = col4row[i];
    } else {   // the solver's rows are the caller's columns: list the pairs by caller row, ascending
        std::vector<int> col_of_row(nr, -1);
        for (int j = 0; j < nc; ++j) col_of_row[col4row[j]] = j;
        int n = 0;
        for (int i = 0; i < nr; ++i)
            if (col_of_row[i] >= 0) rows[n] = i, cols[n] = col_of_row[i], ++n;
    }
    return true;
}
