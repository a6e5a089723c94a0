// Checks every helper of kt_wave.h against the __shfl_xor butterfly it stands
// for, on random bit patterns (xorshift64), 4,096 waves:
//   bits 1, 2, 4  kt::shfl_xor_{u64,i,d} vs __shfl_xor(v, o, 64), o = 1 .. 32, by bits
//   bit 8         a full butterfly sum built from kt::shfl_xor_d, by bits
//   bit 16        kt::wave_sum64, by bits
//   bits 32, 64   kt::wave_minmax64<false / true>, by value
//   bit 128       kt::group_min_i for g = 1, 2, 4, ..., 64
//   bit 256       kt::readlane_d vs __shfl(v, l, 64), by bits
// Prints one JSON line; exit status 0 iff mismatch_mask == 0.
// Build: make -C tests/native/wave_check; needs a gfx950 GPU to run.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../../krylov_robustness_amd/csrc/kt_wave.h"

__device__ bool same_bits(double x, double y) { return __double_as_longlong(x) == __double_as_longlong(y); }

__global__ void k_check(const unsigned long long* in, int* bad) {
    const int l = threadIdx.x;
    const unsigned long long b = in[blockIdx.x * 64 + l];
    const double v = __longlong_as_double((long long)(b & 0x7FEFFFFFFFFFFFFFull));   // finite, >= 0
    const double sv = __longlong_as_double((long long)(b & 0xFFEFFFFFFFFFFFFFull));  // finite, either sign
    int nb = 0;
    for (int o = 1; o < 64; o <<= 1) {
        if (kt::shfl_xor_u64(b, o) != (unsigned long long)__shfl_xor(b, o, 64)) nb |= 1;
        if (kt::shfl_xor_i((int)b, o) != __shfl_xor((int)b, o, 64)) nb |= 2;
        if (!same_bits(kt::shfl_xor_d(v, o), __shfl_xor(v, o, 64))) nb |= 4;
    }
    double s1 = v, s2 = v, mn = sv, mx = sv;
    for (int o = 32; o > 0; o >>= 1) {
        s1 += kt::shfl_xor_d(s1, o);
        s2 += __shfl_xor(s2, o, 64);
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    if (!same_bits(s1, s2)) nb |= 8;
    if (!same_bits(kt::wave_sum64(v), s2)) nb |= 16;
    // by value: the two forms hand fmin / fmax their operands in different
    // orders, so a tie between +0 and -0 may come out with either sign
    if (!(kt::wave_minmax64<false>(sv) == mn)) nb |= 32;
    if (!(kt::wave_minmax64<true>(sv) == mx)) nb |= 64;
    for (int g = 1; g <= 64; g <<= 1) {
        int r = (int)(b >> 17);
        for (int o = 1; o < g; o <<= 1) r = min(r, __shfl_xor(r, o, 64));
        if (kt::group_min_i((int)(b >> 17), g) != r) nb |= 128;
    }
    const int src = blockIdx.x & 63;  // wave-uniform source lane
    if (!same_bits(kt::readlane_d(sv, src), __shfl(sv, src, 64))) nb |= 256;
    if (nb) atomicOr(bad, nb);
}

int main() {
    const int blocks = 4096;
    unsigned long long* h = (unsigned long long*)malloc(sizeof(unsigned long long) * 64 * blocks);
    unsigned long long x = 88172645463325252ull;
    for (int i = 0; i < 64 * blocks; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        h[i] = x;
    }
    unsigned long long* d;
    int *db, hb = 0;
    if (hipMalloc(&d, sizeof(unsigned long long) * 64 * blocks) != hipSuccess || hipMalloc(&db, sizeof(int)) != hipSuccess)
        return 2;
    if (hipMemcpy(d, h, sizeof(unsigned long long) * 64 * blocks, hipMemcpyHostToDevice) != hipSuccess) return 2;
    if (hipMemset(db, 0, sizeof(int)) != hipSuccess) return 2;
    k_check<<<blocks, 64>>>(d, db);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    if (hipMemcpy(&hb, db, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 3;
    printf("{\"wave_check\": \"%s\", \"mismatch_mask\": %d, \"lanes\": %d}\n", hb ? "FAIL" : "ok", hb, 64 * blocks);
    return hb ? 1 : 0;
}
