// Stand-alone host program for the sanitizers: runs the solver of csrc/lsap.h (what fnp_host_lsap calls) on tie-heavy,
// duplicated-column and degenerate matrices of both orientations and checks that every answer is a full matching with
// in-range, distinct indices.  Equality with scipy is tests/test_assign_ref.py's job; this one is for the memory and
// undefined-behaviour checkers, on the CPU only:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lsap_sanitize.cpp -o /tmp/lsap_sanitize
//   /tmp/lsap_sanitize
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../findnpropagate_amd/csrc/lsap.h"

static uint32_t state = 12345u;
static uint32_t next_u32() { return state = state * 1664525u + 1013904223u; }

static int run(int nr, int nc, int levels, bool dup) {
    std::vector<float> cost((size_t)nr * nc);
    for (auto &c : cost) c = levels ? (float)((next_u32() >> 16) % levels) : (float)(next_u32() >> 8) / 16777216.f;
    if (dup && nc > 1)
        for (int k = 0; k < nc / 4 + 1; ++k) {
            const int a = (next_u32() >> 8) % nc, b = (next_u32() >> 8) % nc;
            for (int i = 0; i < nr; ++i) cost[(size_t)i * nc + a] = cost[(size_t)i * nc + b];
        }
    const int n = nr < nc ? nr : nc;
    std::vector<int> rows(n, -1), cols(n, -1);
    if (!fnp_lsap(cost.data(), nr, nc, rows.data(), cols.data())) return 1;
    std::vector<char> seen_r(nr, 0), seen_c(nc, 0);
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] >= nr || cols[i] < 0 || cols[i] >= nc || seen_r[rows[i]] || seen_c[cols[i]]) return 2;
        if (i && rows[i] <= rows[i - 1]) return 3;
        seen_r[rows[i]] = seen_c[cols[i]] = 1;
    }
    return 0;
}

int main() {
    int cases = 0;
    const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 7}, {40, 13}, {13, 40}, {200, 37}, {200, 60}, {64, 70}, {65, 64}};
    for (const auto &s : shapes)
        for (int levels : {0, 1, 2, 3, 4})          // 0: distinct values; 1: a constant matrix; 2..4: {0..levels-1}
            for (bool dup : {false, true}) {
                const int rc = run(s[0], s[1], levels, dup);
                if (rc) {
                    std::printf("FAIL %d x %d levels %d dup %d: %d\n", s[0], s[1], levels, (int)dup, rc);
                    return 1;
                }
                ++cases;
            }
    {   // non-finite costs are out of contract: the solver must return, and say so
        std::vector<float> bad(12, __builtin_inff());
        int r[3], c[3];
        if (fnp_lsap(bad.data(), 3, 4, r, c)) return 1;
        for (auto &x : bad) x = __builtin_nanf("");
        (void)fnp_lsap(bad.data(), 4, 3, r, c);
    }
    std::printf("lsap_sanitize: %d cases clean\n", cases);
    return 0;
}
