// sw_wave.h -- what the one-wave-per-item kernels (batch, search, affine search, alignment) share below their recurrences (gfx950):
// the dropped buffer offset, the sc1 bit and the window size of the alignment kernels, the DPP moves, the profile row load / direction
// row store and the compile-time loop.  Everything is __forceinline__ inside an unnamed namespace: linkage stays internal to the
// translation unit and nothing leaves a symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace swk {

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef int sw_v4i __attribute__((ext_vector_type(4)));
typedef int sw_v2i __attribute__((ext_vector_type(2)));

constexpr u32 SW_OOB = 0xFFFFFF00u;     // buffer offset beyond every descriptor: the access is dropped (loads return 0)
constexpr int SW_SC1 = 16;              // aux bit of the buffer builtins: sc1 (the alignment kernels read their own slot past the L1)
constexpr int SW_WIN = 64;              // the alignment walk's window: SW_WIN rows of SW_WIN direction bytes per wave (sw_align_walk.inc)

__device__ __forceinline__ int sw_dpp_shr1(int old, int src) {   // lane l <- lane l-1; lane 0 keeps `old`
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int sw_sbyte(u32 w, int j) { return (int)(signed char)(w >> (8 * j)); }

__device__ __forceinline__ int sw_wave_max(int v) {   // max over the 64 lanes, wave-uniform result (v >= 0)
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));   // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));   // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));   // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));   // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true));   // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true));   // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

// the C profile bytes of one lane and row (C / 4 dwords)
template <int C>
__device__ __forceinline__ void sw_load_row(__amdgpu_buffer_rsrc_t r, u32 off, u32 (&s)[C / 4]) {
    if constexpr (C == 16) {
        const sw_v4i v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y; s[2] = (u32)v.z; s[3] = (u32)v.w;
    } else if constexpr (C == 8) {
        const sw_v2i v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
        s[0] = (u32)v.x; s[1] = (u32)v.y;
    } else {
        s[0] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0);
    }
}
// the C direction bytes of one lane and row
template <int C>
__device__ __forceinline__ void sw_store_row(__amdgpu_buffer_rsrc_t r, u32 off, const u32 (&d)[C / 4]) {
    if constexpr (C == 16) __builtin_amdgcn_raw_buffer_store_b128(sw_v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]}, r, (int)off, 0, 0);
    else if constexpr (C == 8) __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{(int)d[0], (int)d[1]}, r, (int)off, 0, 0);
    else __builtin_amdgcn_raw_buffer_store_b32((int)d[0], r, (int)off, 0, 0);
}

// f(integral_constant<I>) ... f(integral_constant<N - 1>): a loop whose index is a constant expression in the body
template <int I, int N, typename F>
__device__ __forceinline__ void sw_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sw_for<I + 1, N>(f);
    }
}

// a value every lane holds alike, told to the compiler: it lands in scalar registers
__device__ __forceinline__ int sw_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t sw_uniform64(int64_t v) {
    return (int64_t)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)((u64)v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)(u64)v));
}

}  // namespace

}  // namespace swk
