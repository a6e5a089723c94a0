// host_san -- TEST INFRASTRUCTURE: the host-only parts of the window loop the
// three MIOBI drivers share (kt_miobi_host.h: miobi_edge_window, the window
// length of the two edge drivers, and miobi_step_in_window, the check of the
// device's step count); built by `make host_san` with
// -fsanitize=address,undefined and run on the CPU.  Exit status 0: all agree.
// (miobi_node_window, the node driver's rule, is in ../miobi_node_check.)
#include <cstdio>

#include "kt_miobi_host.h"

static int check(bool ok, const char* what) {
    if (!ok) printf("FAILED: %s\n", what);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    // up to the next multiple of refresh, never past the end; refresh <= 0: one window
    bool ok = kt::miobi_edge_window(24, 0, 0) == 24 && kt::miobi_edge_window(7, 17, -3) == 7 &&      // refresh <= 0
              kt::miobi_edge_window(5, 0, 1) == 1 && kt::miobi_edge_window(2, 3, 1) == 1 &&          // refresh = 1
              kt::miobi_edge_window(5, 0, 100) == 5 && kt::miobi_edge_window(1, 0, 8) == 1 &&        // refresh > remaining
              kt::miobi_edge_window(24, 0, 8) == 8 && kt::miobi_edge_window(16, 8, 8) == 8 &&        // done on a multiple
              kt::miobi_edge_window(21, 3, 8) == 5 && kt::miobi_edge_window(3, 21, 8) == 3;          // done off a multiple
    // the windows of a whole run tile [0, k) and every one but the last ends on a multiple of refresh
    for (int refresh : {-1, 0, 1, 3, 8, 50, 100})
        for (int k : {0, 1, 5, 24, 100}) {
            int done = 0, windows = 0;
            while (done < k) {
                const int w = kt::miobi_edge_window(k - done, done, refresh);
                ok = ok && w >= 1 && done + w <= k && (done + w == k || (refresh > 0 && (done + w) % refresh == 0));
                done += w, ++windows;
            }
            ok = ok && windows == (k == 0 ? 0 : refresh > 0 ? (k - 1) / refresh + 1 : 1);
        }
    bad += check(ok, "miobi_edge_window");
    bad += check(kt::miobi_step_in_window(5, 5, 3) && kt::miobi_step_in_window(8, 5, 3) &&
                     !kt::miobi_step_in_window(4, 5, 3) && !kt::miobi_step_in_window(9, 5, 3) &&
                     kt::miobi_step_in_window(0, 0, 0) && !kt::miobi_step_in_window(-1, 0, 0),
                 "miobi_step_in_window");
    printf("%s\n", bad ? "host_san: FAILED" : "host_san: ok");
    return bad ? 1 : 0;
}
