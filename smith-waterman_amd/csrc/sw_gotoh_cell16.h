// sw_gotoh_cell16.h -- what the kernels that include sw_gotoh_sweep16.inc share beside it (gfx950): the packed maxima, the cell pair
// GS16_CELL2 / gs16_cell2 and the store of one pair's result.  The header of sw_search_multi16.hip argues the cell and its bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sw_kernels.h"
#include "sw_wave.h"

namespace swk {

typedef short gs16_v2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 gs16_max(u32 a, u32 b) {   // v_pk_max_i16
    return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(gs16_v2s, a), __builtin_bit_cast(gs16_v2s, b)));
}
__device__ __forceinline__ u32 gs16_min(u32 a, u32 b) {   // v_pk_min_i16
    return __builtin_bit_cast(u32, __builtin_elementwise_min(__builtin_bit_cast(gs16_v2s, a), __builtin_bit_cast(gs16_v2s, b)));
}

// The columns k (byte BLO of the row dwords) and k + 1 (byte BHI) of both targets as ONE statement.
// %0 hn0, %1 hn1: t, then H of the two columns (out);  %2: x;  %3 e0, %4 e1, %5 f (in / out);  %6: the diagonal of column k, %7: the
// old H of column k = the diagonal of column k + 1;  %8 / %9: the profile dwords of A's and B's row;  %10 goe, %11 ge in both halves.
#define GS16_CELL2(BLO, BHI)                                                                                                          \
    asm("v_add_u32_sdwa %0, %6, sext(%8) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:" BLO "\n\t"                     \
        "v_add_u32_sdwa %1, %7, sext(%8) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:" BHI "\n\t"                     \
        "v_add_u32_sdwa %0, %6, sext(%9) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:" BLO "\n\t"                \
        "v_add_u32_sdwa %1, %7, sext(%9) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:" BHI "\n\t"                \
        "v_pk_max_i16 %0, %0, %3\n\t"                                                                                                 \
        "v_pk_max_i16 %0, %0, %5\n\t"                                                                                                 \
        "v_pk_max_i16 %0, %0, 0\n\t"                                                                                                  \
        "v_pk_add_i16 %2, %0, %10\n\t"                                                                                                \
        "v_pk_add_i16 %3, %3, %11\n\t"                                                                                                \
        "v_pk_add_i16 %5, %5, %11\n\t"                                                                                                \
        "v_pk_max_i16 %3, %3, %2\n\t"                                                                                                 \
        "v_pk_max_i16 %5, %5, %2\n\t"                                                                                                 \
        "v_pk_max_i16 %1, %1, %4\n\t"                                                                                                 \
        "v_pk_max_i16 %1, %1, %5\n\t"                                                                                                 \
        "v_pk_max_i16 %1, %1, 0\n\t"                                                                                                  \
        "v_pk_add_i16 %2, %1, %10\n\t"                                                                                                \
        "v_pk_add_i16 %4, %4, %11\n\t"                                                                                                \
        "v_pk_add_i16 %5, %5, %11\n\t"                                                                                                \
        "v_pk_max_i16 %4, %4, %2\n\t"                                                                                                 \
        "v_pk_max_i16 %5, %5, %2"                                                                                                     \
        : "=&v"(hn0), "=&v"(hn1), "=&v"(x), "+v"(e0), "+v"(e1), "+v"(f) : "v"(dprev), "v"(hk), "v"(SA), "v"(SB), "s"(goe2), "s"(ge2))
template <int J>
__device__ __forceinline__ void gs16_cell2(u32& hn0, u32& hn1, u32 dprev, u32 hk, u32& e0, u32& e1, u32& f, u32 SA, u32 SB, u32 goe2, u32 ge2) {
    static_assert(J == 0 || J == 2, "the lower byte of a pair");
    u32 x;
    if constexpr (J == 2) GS16_CELL2("BYTE_2", "BYTE_3");
    else GS16_CELL2("BYTE_0", "BYTE_1");
}

// lane 0 stores one pair's result: max_pos, max_score, path_len = 0 (the stores of sw_search_affine_multi_wave)
__device__ __forceinline__ void gs16_store(sw_result* at, u64 kbest, u32 voffL0) {
    const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc((void*)at, 0, (int)sizeof(sw_result), 0x00020000);
    const u64 score = kbest >> 40, pos = kbest ? SW_KEY_IDX_MASK - (kbest & SW_KEY_IDX_MASK) : 0;
    const sw_v4i v = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
    __builtin_amdgcn_raw_buffer_store_b128(v, rR, (int)voffL0, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{0, 0}, rR, (int)voffL0, 16, 0);
}

}  // namespace swk
