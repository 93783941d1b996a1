// Wave-level primitives shared by the codec kernels (device only; gfx950, wave64).  Everything is
// __forceinline__ and lives in an anonymous namespace: each translation unit gets its own copies.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mx {

namespace {

// Cross-row exchanges without LDS (CDNA4 v_permlane16/32_swap with both operands = v): the
// swapped pair holds {v, v ^ 16} (resp. {v, v ^ 32}) in some order on every lane, so their
// sum / max / or is the xor-16 (xor-32) step of a butterfly -- no ds_bpermute round trip.
__device__ __forceinline__ void xrow16(uint32_t v, uint32_t& a, uint32_t& b) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    a = r[0];
    b = r[1];
}
__device__ __forceinline__ void xrow32(uint32_t v, uint32_t& a, uint32_t& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    a = r[0];
    b = r[1];
}
// Sum of the four rows of 16 lanes, every lane gets it (whole wave active).
__device__ __forceinline__ uint32_t rows_sum(uint32_t v) {
    uint32_t a, b;
    xrow16(v, a, b);
    xrow32(a + b, a, b);
    return a + b;
}
// Wave sum / max / or, every lane gets it (called with the whole wave active): quad and row-of-16
// steps with DPP (quad_perm [1,0,3,2], [2,3,0,1], row_ror 4, row_ror 8), then the four rows with the
// two permlane swaps -- all VALU, no LDS latency on the (often serial) reduction chains.
__device__ __forceinline__ int wave_sum(int v) {
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false);
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false);
    v += __builtin_amdgcn_mov_dpp(v, 0x124, 0xF, 0xF, false);
    v += __builtin_amdgcn_mov_dpp(v, 0x128, 0xF, 0xF, false);
    return (int)rows_sum((uint32_t)v);
}
__device__ __forceinline__ int wave_max(int v) {
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x124, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x128, 0xF, 0xF, false));
    uint32_t a, b;
    xrow16((uint32_t)v, a, b);
    v = max((int)a, (int)b);
    xrow32((uint32_t)v, a, b);
    return max((int)a, (int)b);
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
    v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);
    v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false);
    v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false);
    uint32_t a, b;
    xrow16(v, a, b);
    xrow32(a | b, a, b);
    return a | b;
}
// Wave minimum of a 64-bit key, every lane gets it: an xor-shuffle ladder (two dwords per step).
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}

// LDS hand-off between the lanes of ONE wave (its own LDS writes visible to its own later reads;
// LDS operations of a wave complete in order): no workgroup barrier, so the waves of a workgroup
// may take different branches around it.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane K of this lane's quad (DPP quad_perm [K,K,K,K]), and the quad's sum on each of its lanes.
template <int K>
__device__ __forceinline__ int qbc(int v) {
    return __builtin_amdgcn_mov_dpp(v, K * 0x55, 0xF, 0xF, false);
}
__device__ __forceinline__ int quad_sum(int v) { return qbc<0>(v) + qbc<1>(v) + qbc<2>(v) + qbc<3>(v); }

// Inclusive prefix sum over the wave's lanes.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// Exclusive scan of v under op (identity `init`) over a workgroup of kThreads threads, all of them
// calling; wbuf: kThreads / 64 values of LDS, free again on return.  *total: the whole workgroup's.
template <int kThreads, typename T, typename Op>
__device__ __forceinline__ T blk_excl_scan(T v, T init, Op op, T* wbuf, T* total) {
    constexpr int kW = kThreads / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(incl, o, 64);
        if (lane >= o) incl = op(incl, t);
    }
    T excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = init;
    if (lane == 63) wbuf[w] = incl;
    __syncthreads();
    T before = init, all = init;
    for (int k = 0; k < kW; ++k) {
        if (k < w) before = op(before, wbuf[k]);
        all = op(all, wbuf[k]);
    }
    __syncthreads();
    *total = all;
    return op(before, excl);
}

}  // namespace

}  // namespace mx
