// host_san -- TEST INFRASTRUCTURE: the host rule of kt_diag_fun_bracket
// (kt_dense.cpp kt_host_gauss_radau / gauss_radau_sums) at the depths 1, 2, 3,
// 168, 169, 255 and 256 -- the largest allocates and solves a 257 x 257
// problem -- on the path graph, where exp(A)_11 of the semi-infinite path is
// known, with a breakdown, with a mu below the Ritz values and with bad
// arguments; built by `make host_san` with -fsanitize=address,undefined and run
// on the CPU.  Exit status 0: all agree.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "kt_internal.h"

namespace kt {
void set_error(const std::string&) {}
}

static int check(bool ok, const char* what) {
    if (!ok) printf("FAILED: %s\n", what);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    // exp(A)_11 of the semi-infinite path = I_0(2) - I_2(2) = I_1(2) by the Bessel series
    double exact = 0.0, term = 1.0;
    for (int k = 0; k < 40; ++k) {
        exact += term / (k + 1);
        term /= (double)(k + 1) * (k + 1);
    }
    for (int j : {1, 2, 3, 168, 169, 255, 256}) {
        // exactly j entries each: one read past them is an ASan report
        std::vector<double> al(j, 0.0), off(j > 1 ? j - 1 : 1, 1.0);
        double lo = 0.0, hi = 0.0;
        int flag = -1;
        const int st = kt_host_gauss_radau(j, al.data(), j > 1 ? off.data() : nullptr, 1.0, 2.5, &lo, &hi, &flag);
        bad += check(st == KT_OK && flag == 0, "status and flag on the path graph");
        bad += check(lo <= exact * (1.0 + 1e-13) && exact <= hi * (1.0 + 1e-13), "lo <= I_1(2) <= hi");
        if (j >= 12) bad += check(hi - lo <= 1e-12 * lo, "the bracket has closed by depth 12");
        int f1 = -1, f2 = -1;
        kt_host_gauss_radau(j, al.data(), j > 1 ? off.data() : nullptr, 0.0, 2.5, &lo, &hi, &f1);
        bad += check(f1 == 1 && hi == lo, "beta_j = 0: flag 1, hi = lo");
        kt_host_gauss_radau(j, al.data(), j > 1 ? off.data() : nullptr, 1.0, -0.5, &lo, &hi, &f2);
        bad += check(f2 == 2 && std::isnan(hi) && lo > 0.0, "mu below the Ritz values: flag 2, hi NaN");
    }
    double lo = 0.0, hi = 0.0, a[2] = {0.0, 0.0};
    int flag = 0;
    bad += check(kt_host_gauss_radau(0, a, a, 1.0, 2.5, &lo, &hi, &flag) == KT_ERR_ARG, "j = 0");
    bad += check(kt_host_gauss_radau(257, a, a, 1.0, 2.5, &lo, &hi, &flag) == KT_ERR_ARG, "j = 257");
    bad += check(kt_host_gauss_radau(2, a, a, 1.0, 701.0, &lo, &hi, &flag) == KT_ERR_ARG, "mu > 700");
    bad += check(kt_host_gauss_radau(2, a, nullptr, 1.0, 2.5, &lo, &hi, &flag) == KT_ERR_ARG, "NULL off");
    printf("%s\n", bad ? "host_san: FAILED" : "host_san: ok");
    return bad ? 1 : 0;
}
