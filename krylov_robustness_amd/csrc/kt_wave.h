// kt_wave.h -- exchanges and reductions between the lanes of one wave64.
//
// PRECONDITION, for every function here but wave_sync: call in wave-uniform
// control flow only (all 64 lanes active, `o`, `g` and `l` the same in every
// lane).  The DPP and permlane moves read the other lanes' registers whatever
// their exec bit, so a lane that branched away hands over a stale value.
//
// KT_WAVE_DPP = 1 (the default on gfx950, whose v_permlane16/32_swap_b32 the
// forms need) moves the partners without the LDS crossbar; 0 (every other
// target, or -DKT_WAVE_DPP=0) builds the __shfl_xor forms, which compile to
// one ds_bpermute_b32 -- an LDS round trip through the pipe the kernels'
// gathers and reductions also use -- per 32-bit half and step.  Both forms
// pair the same lanes: same bits out (tests/native/wave_check checks each
// helper against the __shfl_xor butterfly on random bits; results on other
// targets are not tested, only that the fallback compiles).
#pragma once
#include <hip/hip_runtime.h>

#ifndef KT_WAVE_DPP
#if defined(__gfx950__)
#define KT_WAVE_DPP 1
#else
#define KT_WAVE_DPP 0
#endif
#endif
#if KT_WAVE_DPP && defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "KT_WAVE_DPP=1 needs gfx950 (v_permlane16/32_swap_b32)"
#endif

namespace kt {

#if KT_WAVE_DPP
// lane ^ o's value: o = 1, 2 are DPP quad_perm, o = 4 two DPP row shifts
// merged by bank masks (banks 0 and 2 take lane i + 4, banks 1 and 3 lane
// i - 4), o = 8 DPP row_ror:8, o = 16 / 32 the permlane swaps (the swap hands
// every lane its partner's value in one of its two results)
__device__ __forceinline__ unsigned xor_lane_u32(unsigned v, int o) {
    switch (o) {
        case 1:
            return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
        case 2:
            return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
        case 4: {
            const int t = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xF, 0x5, false);  // row_shl:4, banks 0, 2
            return (unsigned)__builtin_amdgcn_update_dpp(t, (int)v, 0x114, 0xF, 0xA, false);     // row_shr:4, banks 1, 3
        }
        case 8:
            return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
        case 16: {
            const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
            return (__lane_id() & 16) ? r[0] : r[1];
        }
        default: {  // 32
            const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
            return (__lane_id() & 32) ? r[0] : r[1];
        }
    }
}
#endif

// ---- __shfl_xor(v, o, 64), o a power of two <= 32 --------------------------
__device__ __forceinline__ double shfl_xor_d(double v, int o) {
#if KT_WAVE_DPP
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = xor_lane_u32((unsigned)b, o), hi = xor_lane_u32((unsigned)(b >> 32), o);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
#else
    return __shfl_xor(v, o, 64);
#endif
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
#if KT_WAVE_DPP
    const unsigned lo = xor_lane_u32((unsigned)v, o), hi = xor_lane_u32((unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
#else
    return __shfl_xor(v, o, 64);
#endif
}

__device__ __forceinline__ int shfl_xor_i(int v, int o) {
#if KT_WAVE_DPP
    return (int)xor_lane_u32((unsigned)v, o);
#else
    return __shfl_xor(v, o, 64);
#endif
}

__device__ __forceinline__ double shfl_xor(double v, int o) { return shfl_xor_d(v, o); }
__device__ __forceinline__ unsigned long long shfl_xor(unsigned long long v, int o) { return shfl_xor_u64(v, o); }
__device__ __forceinline__ int shfl_xor(int v, int o) { return shfl_xor_i(v, o); }

// ---- whole-wave reductions: the xor butterfly o = 32, 16, ..., 1, the result
// in every lane.  The DPP form takes o = 32, 16 by the permlane swaps (the swap
// hands every lane its own and its partner's half: lo + hi is own + partner up
// to the order of the operands, which fp64 addition ignores), o = 8 by
// row_ror:8 (= lane ^ 8 within a row of 16), o = 4 by row_ror:4 (lane
// (i - 4) mod 16 holds the same value as lane i ^ 4 once the o = 8 step made
// lanes i and i ^ 8 equal), o = 2, 1 by quad_perm.  Every lane adds the same
// pairs as the shuffle form: bit-identical sums.
#if KT_WAVE_DPP
template <int CTRL>
__device__ __forceinline__ double mov_dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <bool B32>
__device__ __forceinline__ double swap_sum_d(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const auto rl = B32 ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                        : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = B32 ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                        : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double x0 = __longlong_as_double(((long long)rh[0] << 32) | (unsigned int)rl[0]);
    const double x1 = __longlong_as_double(((long long)rh[1] << 32) | (unsigned int)rl[1]);
    return x0 + x1;
}
template <bool MAX, bool B32>
__device__ __forceinline__ double swap_mm_d(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const auto rl = B32 ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                        : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = B32 ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                        : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double x0 = __longlong_as_double(((long long)rh[0] << 32) | (unsigned int)rl[0]);
    const double x1 = __longlong_as_double(((long long)rh[1] << 32) | (unsigned int)rl[1]);
    return MAX ? fmax(x0, x1) : fmin(x0, x1);
}
#endif

__device__ __forceinline__ double wave_sum64(double v) {
#if KT_WAVE_DPP
    v = swap_sum_d<true>(v);
    v = swap_sum_d<false>(v);
    v += mov_dpp_d<0x128>(v);  // row_ror:8
    v += mov_dpp_d<0x124>(v);  // row_ror:4
    v += mov_dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
    v += mov_dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
#endif
    return v;
}

// min / max over the wave (exact and commutative: any pairing gives the
// shuffle butterfly's value), same moves as wave_sum64
template <bool MAX>
__device__ __forceinline__ double wave_minmax64(double v) {
#if KT_WAVE_DPP
    v = swap_mm_d<MAX, true>(v);
    v = swap_mm_d<MAX, false>(v);
    v = MAX ? fmax(v, mov_dpp_d<0x128>(v)) : fmin(v, mov_dpp_d<0x128>(v));
    v = MAX ? fmax(v, mov_dpp_d<0x124>(v)) : fmin(v, mov_dpp_d<0x124>(v));
    v = MAX ? fmax(v, mov_dpp_d<0x4E>(v)) : fmin(v, mov_dpp_d<0x4E>(v));
    v = MAX ? fmax(v, mov_dpp_d<0xB1>(v)) : fmin(v, mov_dpp_d<0xB1>(v));
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = MAX ? fmax(v, __shfl_xor(v, o, 64)) : fmin(v, __shfl_xor(v, o, 64));
#endif
    return v;
}

// min over the aligned group of g lanes (g a power of two <= 64)
__device__ __forceinline__ int group_min_i(int v, int g) {
#if KT_WAVE_DPP
    if (g > 1) v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false));  // lane ^ 1
    if (g > 2) v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false));  // lane ^ 2
    if (g > 4) v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false)); // 7 - i: the other quad
    if (g > 8) v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false)); // 15 - i: the other 8
    if (g > 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        v = min((int)r[0], (int)r[1]);
    }
    if (g > 32) {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
        v = min((int)r[0], (int)r[1]);
    }
#else
    for (int o = 1; o < g; o <<= 1) v = min(v, __shfl_xor(v, o, 64));
#endif
    return v;
}

// lane l's double, broadcast to the wave: two v_readlane, no LDS
__device__ __forceinline__ double readlane_d(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// LDS hand-off between the lanes of ONE wave (for code whose waves run
// data-dependent control flow, so no workgroup barrier is possible)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace kt
