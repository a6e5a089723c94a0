// host_san -- TEST INFRASTRUCTURE: the host rule of kt_entries_fun_bracket
// (kt_dense.cpp gauss_radau_sums on both columns, pair_bracket_combine) at the
// depths 1, 2, 3, 168, 169, 255 and 256 on two path graphs, whose entries are
// Bessel series, and every flag of the combine step; built by `make host_san`
// with -fsanitize=address,undefined and run on the CPU.  Exit status 0: all agree.
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

// exp(T)_11 of the semi-infinite path with off-diagonal b: I_1(2b) / b
static double path11(double b) {
    double s = 0.0, term = 1.0;
    for (int k = 0; k < 40; ++k) {
        s += term / (k + 1);
        term *= b * b / ((double)(k + 1) * (k + 1));
    }
    return s;
}

int main() {
    int bad = 0;
    const double mu = 2.5, gp = path11(1.0), gm = path11(0.5), exact = 0.5 * (gp - gm) * std::exp(-mu);
    for (int j : {1, 2, 3, 168, 169, 255, 256}) {
        // exactly j entries each: one read past them is an ASan report
        std::vector<double> al(j, 0.0), op(j, 1.0), om(j, 0.5);
        double Lp, Up, Lm, Um, lo, hi;
        const int kp = kt::gauss_radau_sums(j, al.data(), op.data(), 1.0, mu, &Lp, &Up);
        const int km = kt::gauss_radau_sums(j, al.data(), om.data(), 0.5, mu, &Lm, &Um);
        int f = kt::pair_bracket_combine(Lp, Up, kp, Lm, Um, km, 1e-10, 1e-12, &lo, &hi);
        // a closed bracket may come out inverted by rounding: that is flag 4, not 0
        bad += check(kp == 0 && km == 0 && (f == 0 || f == 3 || (f == 4 && hi < lo)), "two running columns");
        bad += check(lo <= exact + 1e-13 && exact <= hi + 1e-13, "lo <= (I_1(2) - 2 I_1(1)) / 2 <= hi");
        if (j >= 12) bad += check(f != 3 && std::fabs(hi - lo) <= 1e-10 * lo, "the bracket has closed by depth 12");
        // the same form in both columns: the entry is 0, never flag 0
        f = kt::pair_bracket_combine(Lp, Up, kp, Lp, Up, kp, 1e-10, 1e-12, &lo, &hi);
        bad += check(lo == -hi && f == (j >= 12 ? 4 : 3), "lo = -hi: flag 4 once the gap is at the floor, else 3");
        f = kt::pair_bracket_combine(Lp, Lp, 1, Lm, Lm, 1, 1e-10, 1e-12, &lo, &hi);
        bad += check(f == 1 && lo == hi && lo == 0.5 * (Lp - Lm), "both frozen: flag 1, lo = hi");
        f = kt::pair_bracket_combine(Lp, NAN, 2, Lm, Lm, 1, 1e-10, 1e-12, &lo, &hi);
        bad += check(f == 2 && std::isnan(lo) && std::isnan(hi), "mu too small in a column: flag 2, NaN");
        f = kt::pair_bracket_combine(Lp, Up, 0, Lm, Lm, 1, 1e-10, 1e-12, &lo, &hi);
        bad += check(f == (j >= 12 ? 0 : 3) && lo <= hi, "one frozen column: the other decides");
        // an inverted bracket of a few ulps of the scale is the floor's
        f = kt::pair_bracket_combine(1.0, 1.0 - 1e-15, 0, 1.0, 1.0 - 1e-15, 0, 1e-10, 1e-12, &lo, &hi);
        bad += check(f == 4 && hi < lo, "an inverted bracket at rounding level: flag 4");
    }
    printf("%s\n", bad ? "host_san: FAILED" : "host_san: ok");
    return bad ? 1 : 0;
}
