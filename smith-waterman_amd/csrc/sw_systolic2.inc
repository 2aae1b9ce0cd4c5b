// sw_systolic2.inc -- the systolic fill with TWO matrix columns per lane (included by sw_systolic.hip, namespace swk).
//
// Why: a chain-bound fill costs  T = rows*tau + strips*(64*tau + hand-off)  (DESIGN.md section 6).  The 64 steps of wave skew and
// the ~1.8 us hand-off per strip are given; the number of strips is not.  Here lane l of strip s owns the adjacent columns
//     A = 126 s + 2 l - 1,   B = 126 s + 2 l          (lane 0: only B = 126 s, the halo column = lane 63's B of strip s-1)
// and works on ONE row r = u - phi - l for both at local step u: half as many strips for 1.2x the step time (the B cell's left
// and diagonal neighbours sit in the same lane; tools/ubench_perm2.hip: 52 clk per step for two cells against 2 x 28.5).
// Per step (7 VALU):  Z += ngap;  P = max3(tB, gB1, Z);  Q = max3(tA, gB1, Z);  tB' = gB1 + sA;  gA' = max(P[l-1], gA1) (DPP);
//                     gB' = max3(Q, gA', Hin);  tA' = gA' + sB          (Hin: lane 0 = this step's halo value, others = the bias)
// Scope of this kernel: one pair, whole matrix or row band (halo row in as a plain row or as granules, last row out as granules), any
// number of rows, H as int32 / int64 / not at all, P as int32 / int8 / not at all (an odd number of columns only with int32 H + P), an
// alphabet of at most 7 letters (found by the kernel's own prologue; more letters: sw_systolic, enqueued behind it, fills).  Row 0 and
// column 0 of H and P are written by the prologue.  Tiles and batches run on sw_systolic.  Protocols (LDS counters, validate-on-use halo,
// self-tagged edge values in edge4, arg-max key) are those of sw_systolic; the importer below is its perm importer with 126-column strips.

constexpr int S2_W = 126;               // columns a strip computes (63 lanes x 2); the strips follow each other every p.s2w columns (126 or 110)
// (the geometry is a template parameter of the kernel, OV = overlapping strips: as a run-time value it cost the 126-column fill 2 %)
template <bool OV> __device__ __forceinline__ constexpr int s2_stride() { return OV ? 110 : S2_W; }
// the lane whose B column is the next strip's halo column (its edge values are the ones exported): 63, or 55 where strips overlap
template <bool OV> __device__ __forceinline__ constexpr int s2_xlane() { return s2_stride<OV>() >> 1; }

// what a strip's producer and its importer waves share
struct S2Side {
    __attribute__((aligned(16))) u32 halo[SY_RH];
    __attribute__((aligned(16))) u32 lowv[128];        // what lanes 1..63 read where lane 0 reads the halo: the launch bias (below every G)
    int topv[128];                                      // H of the row above this strip's columns 126 s .. 126 s + 126 (bands)
    int prod_u, halo_ready, never, pad;
};
struct Sys2Lds {
    __attribute__((aligned(16))) unsigned char ringA[64 * SY_LSTR];
    __attribute__((aligned(16))) unsigned char ringB[64 * SY_LSTR];
    __attribute__((aligned(16))) int cons_blk[8];
    S2Side side;
};

// gA[k] = v(64+k), gB[k] = v(80+k), Hin[k] = v(100+k); tA = v116/v117, tB = v118/v119 (alternating), P v120, Z v121, Q v122
#define P2_STEP(GA, GB, GA1, GB1, TAP, TAN, TBP, TBN, HIN, SA, SB, BYTE)                                                   \
    "v_add_u32 v121, v121, %[ngap]\n\t"                                                                                   \
    "v_max3_i32 v120, " TBP ", " GB1 ", v121\n\t"                                                                         \
    "v_max3_i32 v122, " TAP ", " GB1 ", v121\n\t"                                                                         \
    "v_add_u32_sdwa " TBN ", " GB1 ", sext(" SA ") dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" BYTE "\n\t" \
    "v_max_i32_dpp " GA ", v120, " GA1 " wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"                                       \
    "v_max3_i32 " GB ", v122, " GA ", " HIN "\n\t"                                                                        \
    "v_add_u32_sdwa " TAN ", " GA ", sext(" SB ") dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" BYTE "\n\t"
#define P2_EVEN(GA, GB, GA1, GB1, HIN, SA, SB, BYTE) P2_STEP(GA, GB, GA1, GB1, "v117", "v116", "v119", "v118", HIN, SA, SB, BYTE)
#define P2_ODD(GA, GB, GA1, GB1, HIN, SA, SB, BYTE) P2_STEP(GA, GB, GA1, GB1, "v116", "v117", "v118", "v119", HIN, SA, SB, BYTE)
#define P2_GRP0 P2_EVEN("v64", "v80", "v79", "v95", "v100", "v40", "v44", "BYTE_0") P2_ODD("v65", "v81", "v64", "v80", "v101", "v40", "v44", "BYTE_1")   \
                P2_EVEN("v66", "v82", "v65", "v81", "v102", "v40", "v44", "BYTE_2") P2_ODD("v67", "v83", "v66", "v82", "v103", "v40", "v44", "BYTE_3")
#define P2_GRP1 P2_EVEN("v68", "v84", "v67", "v83", "v104", "v41", "v45", "BYTE_0") P2_ODD("v69", "v85", "v68", "v84", "v105", "v41", "v45", "BYTE_1")   \
                P2_EVEN("v70", "v86", "v69", "v85", "v106", "v41", "v45", "BYTE_2") P2_ODD("v71", "v87", "v70", "v86", "v107", "v41", "v45", "BYTE_3")
#define P2_GRP2 P2_EVEN("v72", "v88", "v71", "v87", "v108", "v42", "v46", "BYTE_0") P2_ODD("v73", "v89", "v72", "v88", "v109", "v42", "v46", "BYTE_1")   \
                P2_EVEN("v74", "v90", "v73", "v89", "v110", "v42", "v46", "BYTE_2") P2_ODD("v75", "v91", "v74", "v90", "v111", "v42", "v46", "BYTE_3")
#define P2_GRP3 P2_EVEN("v76", "v92", "v75", "v91", "v112", "v43", "v47", "BYTE_0") P2_ODD("v77", "v93", "v76", "v92", "v113", "v43", "v47", "BYTE_1")   \
                P2_EVEN("v78", "v94", "v77", "v93", "v114", "v43", "v47", "BYTE_2") P2_ODD("v79", "v95", "v78", "v94", "v115", "v43", "v47", "BYTE_3")
// after group g of a block: the ring writes of its 4 steps, lane 63's edge store, and the halo group g of the NEXT block
#define P2_TAIL(GA0, GA3, GB0, GB3, H0, H3, WO, HADDR)                                                                     \
    "ds_write_b128 v99, v[" GA0 ":" GA3 "] offset:" WO "\n\t"                                                              \
    "ds_write_b128 v123, v[" GB0 ":" GB3 "] offset:" WO "\n\t"                                                             \
    "buffer_store_dwordx4 v[" GB0 ":" GB3 "], v97, s[76:79], s75 offen offset:" WO " sc1\n\t"                               \
    "buffer_store_dwordx4 v[" GB0 ":" GB3 "], %[expoffl], s[76:79], s75 offen offset:" WO " sc0\n\t"                        \
    "ds_read_b128 v[" H0 ":" H3 "], " HADDR "\n\t"
// both halo groups of a pair there <=> the AND of their last values keeps the tag byte (unfilled slots read 0)
#define P2_CHK(V0, V1, LBL)                                                                                                \
    "s_waitcnt lgkmcnt(7)\n\t"                                                                                            \
    "v_readfirstlane_b32 s85, " V0 "\n\t"                                                                                 \
    "v_readfirstlane_b32 s86, " V1 "\n\t"                                                                                 \
    "s_and_b32 s85, s85, s86\n\t"                                                                                         \
    "s_cbranch_scc0 " LBL "\n"
// KB: first step of the block in the chunk; CA*/CB*: code dwords of the block (A' stream and B stream); NA/NB + PF/PF1: buffers
// and byte offsets of the codes of the block two ahead; W*: ring byte offsets of the groups; N*: halo operands of the NEXT
// block's groups; BPF: back-pressure fetch
#define P2_BLOCK(KB, CA0, CA1, CA2, CA3, CB0, CB1, CB2, CB3, NA, NB, PF, PF1, W0, W1, W2, W3, N0, N1, N2, N3, BPF)         \
    P2_CHK("v103", "v107", "LslowA" #KB "_%=")                                                                            \
    "LgoA" #KB "_%=:\n\t"                                                                                                 \
    "s_waitcnt vmcnt(18)\n\t"               /* the codes loaded two blocks ago: 2 loads + 2 x 8 edge stores are younger */   \
    "v_perm_b32 v40, %[pahi], %[palo], " CA0 "\n\t"                                                                       \
    "v_perm_b32 v41, %[pahi], %[palo], " CA1 "\n\t"                                                                       \
    "v_perm_b32 v42, %[pahi], %[palo], " CA2 "\n\t"                                                                       \
    "v_perm_b32 v43, %[pahi], %[palo], " CA3 "\n\t"                                                                       \
    "v_perm_b32 v44, %[pbhi], %[pblo], " CB0 "\n\t"                                                                       \
    "v_perm_b32 v45, %[pbhi], %[pblo], " CB1 "\n\t"                                                                       \
    "v_perm_b32 v46, %[pbhi], %[pblo], " CB2 "\n\t"                                                                       \
    "v_perm_b32 v47, %[pbhi], %[pblo], " CB3 "\n\t"                                                                       \
    "global_load_dwordx4 " NA ", v96, s[92:93] offset:" PF "\n\t"                                                         \
    "global_load_dwordx4 " NB ", v96, s[92:93] offset:" PF1 "\n\t"                                                        \
    P2_GRP0 P2_TAIL("64", "67", "80", "83", "100", "103", W0, N0)                                                         \
    P2_GRP1 P2_TAIL("68", "71", "84", "87", "104", "107", W1, N1)                                                         \
    P2_CHK("v111", "v115", "LslowB" #KB "_%=")                                                                            \
    "LgoB" #KB "_%=:\n\t"                                                                                                 \
    P2_GRP2 P2_TAIL("72", "75", "88", "91", "108", "111", W2, N2)                                                         \
    BPF                                                                                                                   \
    P2_GRP3 P2_TAIL("76", "79", "92", "95", "112", "115", W3, N3)                                                         \
    "v_add_u32 v29, 16, v29\n\t"                                                                                          \
    "ds_write_b32 v31, v29\n\t"
#define P2_BPFETCH "ds_read_b128 v[124:127], v39\n\tds_read_b128 v[32:35], v39 offset:16\n\tds_read_b32 v36, v30\n\t"
// ring back-pressure before the 32 steps that start at local step s88 + D (operands kc / kr carry D)
#define P2_BPCHECK(T, KC, KR)                                                                                             \
    "s_waitcnt lgkmcnt(4)\n\t"                        /* the fetches sit in front of the last group's tail and the progress write */ \
    "v_min3_i32 v37, v124, v125, v126\n\t"                                                                                \
    "v_min3_i32 v38, v127, v32, v33\n\t"                                                                                  \
    "v_min3_i32 v37, v37, v34, v35\n\t"                                                                                   \
    "v_min_i32 v37, v37, v38\n\t"                                                                                         \
    "s_mov_b32 s89, 0\n\t"                                                                                                \
    "v_readfirstlane_b32 s86, v36\n\t"                                                                                    \
    "v_readfirstlane_b32 s85, v37\n"                                                                                      \
    "Lbpe" T "_%=:\n\t"                                                                                                   \
    "s_lshl_b32 s85, s85, 4\n\t"                                                                                          \
    "s_add_i32 s85, s85, 16\n\t"                                                                                          \
    "s_add_i32 s87, s88, " KC "\n\t"                                                                                      \
    "s_cmp_ge_i32 s85, s87\n\t"                                                                                           \
    "s_cbranch_scc0 Lbpw" T "_%=\n\t"                                                                                     \
    "s_add_i32 s87, s88, " KR "\n\t"                                                                                      \
    "s_cmp_ge_i32 s86, s87\n\t"                                                                                           \
    "s_cbranch_scc1 Lbpok" T "_%=\n"                                                                                      \
    "Lbpw" T "_%=:\n\t"                                                                                                   \
    "s_sleep 1\n\t"                                                                                                       \
    "s_add_i32 s89, s89, 1\n\t"                                                                                           \
    "s_add_i32 s94, s94, 1\n\t"                                                                                           \
    "s_cmp_lt_u32 s89, 0x1000000\n\t"                                                                                     \
    "s_cbranch_scc0 Lfail_%=\n\t"                                                                                         \
    "ds_read_b128 v[124:127], v39\n\t"                                                                                    \
    "ds_read_b128 v[32:35], v39 offset:16\n\t"                                                                            \
    "ds_read_b32 v36, v30\n\t"                                                                                            \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                            \
    "v_min3_i32 v37, v124, v125, v126\n\t"                                                                                \
    "v_min3_i32 v38, v127, v32, v33\n\t"                                                                                  \
    "v_min3_i32 v37, v37, v34, v35\n\t"                                                                                   \
    "v_min_i32 v37, v37, v38\n\t"                                                                                         \
    "s_nop 1\n\t"                                                                                                         \
    "v_readfirstlane_b32 s85, v37\n\t"                                                                                    \
    "v_readfirstlane_b32 s86, v36\n\t"                                                                                    \
    "s_branch Lbpe" T "_%=\n"                                                                                             \
    "Lbpok" T "_%=:\n\t"
// out of line: fetch a pair of halo groups again until both are there
#define P2_SLOW(KB, R0, R1, R2, R3)                                                                                       \
    "LslowA" #KB "_%=:\n\t"                                                                                               \
    "s_mov_b32 s89, 0\n"                                                                                                  \
    "LpollA" #KB "_%=:\n\t"                                                                                               \
    "ds_read_b128 v[100:103], v98 offset:" R0 "\n\t"                                                                      \
    "ds_read_b128 v[104:107], v98 offset:" R1 "\n\t"                                                                      \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                            \
    "v_readfirstlane_b32 s85, v103\n\t"                                                                                   \
    "v_readfirstlane_b32 s86, v107\n\t"                                                                                   \
    "s_and_b32 s85, s85, s86\n\t"                                                                                         \
    "s_cbranch_scc1 LgoA" #KB "_%=\n\t"                                                                                   \
    "s_add_i32 s89, s89, 1\n\t"                                                                                           \
    "s_add_i32 s95, s95, 1\n\t"                                                                                           \
    "s_cmp_lt_u32 s89, 0x1000000\n\t"                                                                                     \
    "s_cbranch_scc1 LpollA" #KB "_%=\n\t"                                                                                 \
    "s_branch Lfail_%=\n"                                                                                                 \
    "LslowB" #KB "_%=:\n\t"                                                                                               \
    "s_mov_b32 s89, 0\n"                                                                                                  \
    "LpollB" #KB "_%=:\n\t"                                                                                               \
    "ds_read_b128 v[108:111], v98 offset:" R2 "\n\t"                                                                      \
    "ds_read_b128 v[112:115], v98 offset:" R3 "\n\t"                                                                      \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                            \
    "v_readfirstlane_b32 s85, v111\n\t"                                                                                   \
    "v_readfirstlane_b32 s86, v115\n\t"                                                                                   \
    "s_and_b32 s85, s85, s86\n\t"                                                                                         \
    "s_cbranch_scc1 LgoB" #KB "_%=\n\t"                                                                                   \
    "s_add_i32 s89, s89, 1\n\t"                                                                                           \
    "s_add_i32 s95, s95, 1\n\t"                                                                                           \
    "s_cmp_lt_u32 s89, 0x1000000\n\t"                                                                                     \
    "s_cbranch_scc1 LpollB" #KB "_%=\n\t"                                                                                 \
    "s_branch Lfail_%=\n"

// ---- consumer: one 16-row block of both columns in ONE asm statement (hipcc's version of the same block: ~750 instructions).
// Literal registers: gA[0..16] = v64..v80, gB[0..16] = v81..v97 (ring entries of rows r0-1 .. r0+15), H pairs v[100:101] /
// v[104:105], P pairs v[102:103] / v[106:107] (alternating rows), v108/v109 scores, v110/v111 diagonal candidates.
// Per row 22 VALU + 2 stores + 1 SALU:  nz -= ngap; hA = gA + nz; hB = gB + nz - ngap; sA/sB by compare + select against the
// row's character (SGPR byte); dA = dpp(gB of the row above, lane l-1) + sA; dB = gA of the row above + sB; P by three
// compares + three selects per cell (serial_smithW.c:204-234: DIAGONAL before UP before LEFT, NONE iff H == 0).
// PST: the P store of the row -- C2_P32 (one dwordx2) or C2_P8 (two bytes: the row pitch is odd, a 2-byte store would be
// misaligned every other row); TRK: C2_TRK records the first cell of the block that beats the lane's best so far (needed when H
// is not written: there is nothing to re-read at the end), or nothing.  K2: 2 * (row index in the block).
#define C2_P32(PA, PB, PP, POL) "buffer_store_dwordx2 " PP ", %[voffP], %[rP], s82 offen" POL "\n\t"
#define C2_P8(PA, PB, PP, POL)                                                                                             \
    "buffer_store_byte " PA ", %[voffP], %[rP], s82 offen" POL "\n\t"                                                      \
    "buffer_store_byte " PB ", %[voffP], %[rP], s82 offen offset:1" POL "\n\t"
#define C2_NOTRK(HA, HB, K2) ""
#define C2_TRK(HA, HB, K2)                                                                                                 \
    "v_cmp_gt_i32_e64 s[72:73], " HA ", %[bv]\n\t"                                                                         \
    "v_max_i32 %[bv], %[bv], " HA "\n\t"                                                                                   \
    "v_cndmask_b32_e64 %[bi], %[bi], " K2 ", s[72:73]\n\t"                                                                 \
    "v_cmp_gt_i32_e64 s[72:73], " HB ", %[bv]\n\t"                                                                         \
    "v_max_i32 %[bv], %[bv], " HB "\n\t"                                                                                   \
    "v_cndmask_b32_e64 %[bi], %[bi], " K2 "+1, s[72:73]\n\t"
#define C2_ROW(GA0, GA1, GB0, GB1, CH, BYTE, HA, HB, HP, PA, PB, PP, POL, HST, PST, TRK, K2)                                    \
    "v_sub_u32 %[nz], %[nz], %[ngap]\n\t"                                                                                 \
    "v_cmp_eq_u32_sdwa s[68:69], %[aA], " CH " src0_sel:DWORD src1_sel:" BYTE "\n\t"                                       \
    "v_cmp_eq_u32_sdwa s[70:71], %[aB], " CH " src0_sel:DWORD src1_sel:" BYTE "\n\t"                                       \
    "v_add_u32 " HA ", " GA1 ", %[nz]\n\t"                                                                                \
    "v_add3_u32 " HB ", " GB1 ", %[nz], v112\n\t"                                                                     \
    "v_cndmask_b32_e64 v113, %[xm], %[mm], s[68:69]\n\t"                                                                  \
    "v_cndmask_b32_e64 v114, %[xm], %[mm], s[70:71]\n\t"                                                                  \
    HST(HP, POL)                                                                                                           \
    "v_cmp_eq_u32_e64 s[60:61], " GA0 ", " GA1 "\n\t"                                                                     \
    "v_cmp_eq_u32_e64 s[64:65], " GB0 ", " GB1 "\n\t"                                                                     \
    "v_add_u32_dpp v115, " GB0 ", v113 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"                            \
    "v_add_u32 v116, " GA0 ", v114\n\t"                                                                                   \
    "v_cndmask_b32_e64 " PA ", 2, 1, s[60:61]\n\t"                                                                        \
    "v_cndmask_b32_e64 " PB ", 2, 1, s[64:65]\n\t"                                                                        \
    "v_cmp_eq_u32_e64 s[62:63], v115, " GA1 "\n\t"                                                                        \
    "v_cmp_eq_u32_e64 s[66:67], v116, " GB1 "\n\t"                                                                        \
    "v_max3_i32 %[bm], %[bm], " HA ", " HB "\n\t"                                                                         \
    "v_cmp_eq_u32_e64 s[68:69], 0, " HA "\n\t"                                                                            \
    "v_cndmask_b32_e64 " PA ", " PA ", 3, s[62:63]\n\t"                                                                   \
    "v_cndmask_b32_e64 " PB ", " PB ", 3, s[66:67]\n\t"                                                                   \
    "v_cmp_eq_u32_e64 s[70:71], 0, " HB "\n\t"                                                                            \
    "s_add_u32 s80, s80, %[rowbH]\n\t"                                                                                    \
    "v_cndmask_b32_e64 " PA ", " PA ", 0, s[68:69]\n\t"                                                                   \
    TRK(HA, HB, K2)                                                                                                        \
    "v_cndmask_b32_e64 " PB ", " PB ", 0, s[70:71]\n\t"                                                                   \
    PST(PA, PB, PP, POL)                                                                                                   \
    "s_add_u32 s82, s82, %[rowbP]\n\t"
// H stores: int32 -- {hA, hB} as one dwordx2; int64 -- {hA, 0, hB, 0} as one dwordx4 (a score is never negative: the high dwords are
// registers that stay zero), i.e. 1008-byte row segments
#define C2_H32(HP, POL) "buffer_store_dwordx2 " HP ", %[voffH], %[rH], s80 offen" POL "\n\t"
#define C2_H64(HP, POL) "buffer_store_dwordx4 " HP ", %[voffH], %[rH], s80 offen" POL "\n\t"
#define C2_EV32(GA0, GA1, GB0, GB1, CH, BYTE, POL, PST, TRK, K2) C2_ROW(GA0, GA1, GB0, GB1, CH, BYTE, "v100", "v101", "v[100:101]", "v102", "v103", "v[102:103]", POL, C2_H32, PST, TRK, K2)
#define C2_OD32(GA0, GA1, GB0, GB1, CH, BYTE, POL, PST, TRK, K2) C2_ROW(GA0, GA1, GB0, GB1, CH, BYTE, "v104", "v105", "v[104:105]", "v106", "v107", "v[106:107]", POL, C2_H32, PST, TRK, K2)
#define C2_EV64(GA0, GA1, GB0, GB1, CH, BYTE, POL, PST, TRK, K2) C2_ROW(GA0, GA1, GB0, GB1, CH, BYTE, "v100", "v102", "v[100:103]", "v104", "v105", "v[104:105]", POL, C2_H64, PST, TRK, K2)
#define C2_OD64(GA0, GA1, GB0, GB1, CH, BYTE, POL, PST, TRK, K2) C2_ROW(GA0, GA1, GB0, GB1, CH, BYTE, "v106", "v108", "v[106:109]", "v110", "v111", "v[110:111]", POL, C2_H64, PST, TRK, K2)
#define C2_RD(K, KB, OFF) "ds_read_b32 v" #K ", %[ea] offset:" #OFF "\n\tds_read_b32 v" #KB ", %[eb] offset:" #OFF "\n\t"
#define C2_RDW(K, KB, I)                                                                                                   \
    "v_add_u32 v98, " #I ", %[ew]\n\t"                                                                                   \
    "v_and_b32 v98, 1020, v98\n\t"                                                                                        \
    "v_add_u32 v99, v98, %[eb]\n\t"                                                                                       \
    "v_add_u32 v98, v98, %[ea]\n\t"                                                                                       \
    "ds_read_b32 v" #K ", v98\n\t"                                                                                        \
    "ds_read_b32 v" #KB ", v99\n\t"
#define C2_READS_FLAT                                                                                                      \
    C2_RD(64, 81, 0) C2_RD(65, 82, 4) C2_RD(66, 83, 8) C2_RD(67, 84, 12) C2_RD(68, 85, 16) C2_RD(69, 86, 20) C2_RD(70, 87, 24) C2_RD(71, 88, 28)      \
    C2_RD(72, 89, 32) C2_RD(73, 90, 36) C2_RD(74, 91, 40) C2_RD(75, 92, 44) C2_RD(76, 93, 48) C2_RD(77, 94, 52) C2_RD(78, 95, 56) C2_RD(79, 96, 60) \
    C2_RD(80, 97, 64)
#define C2_READS_WRAP                                                                                                      \
    C2_RDW(64, 81, 0) C2_RDW(65, 82, 4) C2_RDW(66, 83, 8) C2_RDW(67, 84, 12) C2_RDW(68, 85, 16) C2_RDW(69, 86, 20) C2_RDW(70, 87, 24)              \
    C2_RDW(71, 88, 28) C2_RDW(72, 89, 32) C2_RDW(73, 90, 36) C2_RDW(74, 91, 40) C2_RDW(75, 92, 44) C2_RDW(76, 93, 48) C2_RDW(77, 94, 52)            \
    C2_RDW(78, 95, 56) C2_RDW(79, 96, 60) C2_RDW(80, 97, 64)
// READS: FLAT -- ea / eb = the lane's ring address of row r0-1 (no lane wraps inside the block); WRAP -- ea / eb = the lane's ring
// bases, ew = byte offset of row r0-1 in the ring
#define C2_ASM(READS, POL, PST, TRK, C2_EV, C2_OD)                                                                                       \
    asm volatile(                                                                                                          \
        "s_load_dwordx4 s[76:79], %[cptr], 0x0\n\t"                                                                       \
        READS                                                                                                              \
        "ds_write_b32 %[slot], %[qv]\n\t"           /* behind the reads in LDS order: the producer may reuse the entries */ \
        "s_mov_b32 s80, 0\n\t"                                                                                            \
        "s_mov_b32 s82, 0\n\t"                                                                                            \
        "v_sub_u32 v112, 0, %[ngap]\n\t"                                                                                  \
        "v_mov_b32 v101, 0\n\tv_mov_b32 v103, 0\n\tv_mov_b32 v107, 0\n\tv_mov_b32 v109, 0\n\t"   /* high dwords of an int64 H (overwritten in the int32 forms) */ \
        "s_waitcnt lgkmcnt(0)\n\t"                  /* (scalar loads return out of order: no counting) */                  \
        "s_cmp_lg_u32 %[first], 0\n\t"                                                                                    \
        "s_cbranch_scc0 Lc2_%=\n\t"                                                                                       \
        "v_mov_b32 v64, %[g0a]\n\t"                 /* row 0 is known (and has no ring entry in lane 0 of the last strip) */ \
        "v_mov_b32 v81, %[g0b]\n"                                                                                          \
        "Lc2_%=:\n\t"                                                                                                     \
        C2_EV("v64", "v65", "v81", "v82", "s76", "BYTE_0", POL, PST, TRK, "0") C2_OD("v65", "v66", "v82", "v83", "s76", "BYTE_1", POL, PST, TRK, "2")       \
        C2_EV("v66", "v67", "v83", "v84", "s76", "BYTE_2", POL, PST, TRK, "4") C2_OD("v67", "v68", "v84", "v85", "s76", "BYTE_3", POL, PST, TRK, "6")       \
        C2_EV("v68", "v69", "v85", "v86", "s77", "BYTE_0", POL, PST, TRK, "8") C2_OD("v69", "v70", "v86", "v87", "s77", "BYTE_1", POL, PST, TRK, "10")      \
        C2_EV("v70", "v71", "v87", "v88", "s77", "BYTE_2", POL, PST, TRK, "12") C2_OD("v71", "v72", "v88", "v89", "s77", "BYTE_3", POL, PST, TRK, "14")     \
        C2_EV("v72", "v73", "v89", "v90", "s78", "BYTE_0", POL, PST, TRK, "16") C2_OD("v73", "v74", "v90", "v91", "s78", "BYTE_1", POL, PST, TRK, "18")     \
        C2_EV("v74", "v75", "v91", "v92", "s78", "BYTE_2", POL, PST, TRK, "20") C2_OD("v75", "v76", "v92", "v93", "s78", "BYTE_3", POL, PST, TRK, "22")     \
        C2_EV("v76", "v77", "v93", "v94", "s79", "BYTE_0", POL, PST, TRK, "24") C2_OD("v77", "v78", "v94", "v95", "s79", "BYTE_1", POL, PST, TRK, "26")     \
        C2_EV("v78", "v79", "v95", "v96", "s79", "BYTE_2", POL, PST, TRK, "28") C2_OD("v79", "v80", "v96", "v97", "s79", "BYTE_3", POL, PST, TRK, "30")     \
        "v_mov_b32 %[gla], v80\n\t"                 /* the block's last row (a band's last row leaves as granules) */     \
        "v_mov_b32 %[glb], v97\n\t"                                                                                       \
        : [nz] "+v"(nz), [bm] "+v"(bm), [bv] "+v"(bv), [bi] "+v"(bi), [gla] "=&v"(gla), [glb] "=&v"(glb)                    \
        : [ea] "v"(ea), [eb] "v"(eb), [ew] "v"(ew), [slot] "v"(slot_addr), [qv] "v"(qv), [first] "s"(first), [g0a] "v"(g0a), [g0b] "v"(g0b),  \
          [aA] "v"(aA), [aB] "v"(aB), [mm] "v"(mm_v), [xm] "v"(xm_v), [ngap] "v"(ngap_v), [voffH] "v"(voffH),           \
          [voffP] "v"(voffP), [rH] "s"(rH), [rP] "s"(rP), [rowbH] "s"(rowbH), [rowbP] "s"(rowbP), [cptr] "s"(chars)           \
        : "vcc", "scc", "memory", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s76", "s77", "s78", "s79", \
          "s80", "s82", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82",    \
          "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", \
          "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116")
struct C2Out { u32 bm, gla, glb; };   // block maximum (garbage where a column does not exist); G of the block's last row
// flat: no lane's ring entries wrap inside the block; nt: streaming stores; p8: int8 P; trk: track the cell of the maximum in the
// block (bv / bi: the lane's best so far and 2 * row-in-block + column of the first cell that beat it)
__device__ __forceinline__ C2Out consumer_block2(bool flat, bool nt, bool p8, bool trk, bool h64, u32 ea, u32 eb, u32 ew, u32 slot_addr, u32 qv, int first, u32 g0a,
                                                 u32 g0b, u32& nz, u32& bv, u32& bi, u32 aA, u32 aB, u32 mm_v, u32 xm_v, u32 ngap_v, u32 voffH,
                                                 u32 voffP, sw_i32x4 rH, sw_i32x4 rP, u32 rowbH, u32 rowbP, const unsigned char* chars) {
    u32 bm = 0, gla, glb;
#define C2_PICK(READS)                                                                                                     \
    if (h64) {   /* (int64 H is always written: no tracking form) */                                                        \
        if (p8) { if (nt) { C2_ASM(READS, " nt", C2_P8, C2_NOTRK, C2_EV64, C2_OD64); } else { C2_ASM(READS, "", C2_P8, C2_NOTRK, C2_EV64, C2_OD64); } }        \
        else { if (nt) { C2_ASM(READS, " nt", C2_P32, C2_NOTRK, C2_EV64, C2_OD64); } else { C2_ASM(READS, "", C2_P32, C2_NOTRK, C2_EV64, C2_OD64); } }         \
    } else if (trk) {                                                                                                      \
        if (p8) { if (nt) { C2_ASM(READS, " nt", C2_P8, C2_TRK, C2_EV32, C2_OD32); } else { C2_ASM(READS, "", C2_P8, C2_TRK, C2_EV32, C2_OD32); } }            \
        else { if (nt) { C2_ASM(READS, " nt", C2_P32, C2_TRK, C2_EV32, C2_OD32); } else { C2_ASM(READS, "", C2_P32, C2_TRK, C2_EV32, C2_OD32); } }             \
    } else {                                                                                                               \
        if (p8) { if (nt) { C2_ASM(READS, " nt", C2_P8, C2_NOTRK, C2_EV32, C2_OD32); } else { C2_ASM(READS, "", C2_P8, C2_NOTRK, C2_EV32, C2_OD32); } }        \
        else { if (nt) { C2_ASM(READS, " nt", C2_P32, C2_NOTRK, C2_EV32, C2_OD32); } else { C2_ASM(READS, "", C2_P32, C2_NOTRK, C2_EV32, C2_OD32); } }         \
    }
    if (flat) { C2_PICK(C2_READS_FLAT) } else { C2_PICK(C2_READS_WRAP) }
#undef C2_PICK
    return C2Out{bm, gla, glb};
}

#include "sw_wholeline_consumer.inc"

// UT: a multiple of 64.  hb / lowb: LDS addresses of the halo ring and of the low values; lane0: 1 in lane 0, else 0.
#include "sw_filler_producer.inc"


// ---- the SCOUT: the chain alone.  A fill is bound by the chain of strips, and what slows the chain down is everything else a
// strip's workgroup does: ring writes and back-pressure in the producer, the consumers' LDS reads, and above all their H / P
// stores, behind which the polling loads of the hand-off queue in the CU's memory pipeline.  None of that is needed to KNOW the
// edge columns.  So scout workgroups run the recurrence of every strip once more -- producer and importers only, nothing kept
// but lane 63's column in edge4 -- ahead of the workgroups that write the matrices ("fillers": the classic producer /
// consumer / importer workgroup, one strip each), which now depend on the scouts' edge columns only, not on each other.
// Same step numbering, same values, same edge4 layout as producer_perm2; two strips per scout workgroup.
#define P2S_TAIL(GB0, GB3, H0, H3, WO, HADDR)                                                                              \
    "buffer_store_dwordx4 v[" GB0 ":" GB3 "], v97, s[76:79], s75 offen offset:" WO P2S_EXP_MOD "\n\t"                       \
    "ds_read_b128 v[" H0 ":" H3 "], " HADDR "\n\t"
#define P2S_LGKM "3"
#ifndef P2S_VMCNT
#define P2S_VMCNT "10"
#endif
#define P2S_CHK(V0, V1, LBL)                                                                                               \
    "s_waitcnt lgkmcnt(" P2S_LGKM ")\n\t"                                                                                            \
    "v_readfirstlane_b32 s85, " V0 "\n\t"                                                                                 \
    "v_readfirstlane_b32 s86, " V1 "\n\t"                                                                                 \
    "s_and_b32 s85, s85, s86\n\t"                                                                                         \
    "s_cbranch_scc0 " LBL "\n"
#define P2S_BLOCK(KB, CA0, CA1, CA2, CA3, CB0, CB1, CB2, CB3, NA, NB, PF, PF1, W0, W1, W2, W3, N0, N1, N2, N3)             \
    P2S_CHK("v103", "v107", "LslowA" #KB "_%=")                                                                           \
    "LgoA" #KB "_%=:\n\t"                                                                                                 \
    "s_waitcnt vmcnt(" P2S_VMCNT ")\n\t"                                                                                             \
    "v_perm_b32 v40, %[pahi], %[palo], " CA0 "\n\t"                                                                       \
    "v_perm_b32 v41, %[pahi], %[palo], " CA1 "\n\t"                                                                       \
    "v_perm_b32 v42, %[pahi], %[palo], " CA2 "\n\t"                                                                       \
    "v_perm_b32 v43, %[pahi], %[palo], " CA3 "\n\t"                                                                       \
    "v_perm_b32 v44, %[pbhi], %[pblo], " CB0 "\n\t"                                                                       \
    "v_perm_b32 v45, %[pbhi], %[pblo], " CB1 "\n\t"                                                                       \
    "v_perm_b32 v46, %[pbhi], %[pblo], " CB2 "\n\t"                                                                       \
    "v_perm_b32 v47, %[pbhi], %[pblo], " CB3 "\n\t"                                                                       \
    "global_load_dwordx4 " NA ", v96, s[92:93] offset:" PF "\n\t"                                                         \
    "global_load_dwordx4 " NB ", v96, s[92:93] offset:" PF1 "\n\t"                                                        \
    P2_GRP0 P2S_TAIL("80", "83", "100", "103", W0, N0)                                                                    \
    P2_GRP1 P2S_TAIL("84", "87", "104", "107", W1, N1)                                                                    \
    P2S_CHK("v111", "v115", "LslowB" #KB "_%=")                                                                           \
    "LgoB" #KB "_%=:\n\t"                                                                                                 \
    P2_GRP2 P2S_TAIL("88", "91", "108", "111", W2, N2)                                                                    \
    P2_GRP3 P2S_TAIL("92", "95", "112", "115", W3, N3)                                                                    \
    "v_add_u32 v29, 16, v29\n\t"                                                                                          \
    "ds_write_b32 v31, v29\n\t"

#define P2S_FN producer_scout2
#define P2S_EXP_MOD " sc1"
#include "sw_scout_producer.inc"
#undef P2S_FN
#undef P2S_EXP_MOD
#define P2S_FN producer_scout2_local
#define P2S_EXP_MOD " sc0"
#include "sw_scout_producer.inc"
#undef P2S_FN
#undef P2S_EXP_MOD
#include "sw_scoutfill_producer.inc"

// ---- pieces shared by the filler and the scout roles ------------------------------------------------------------------------
// H of the row above strip s (bands): a plain int32 row, or {tag, H} granules that arrive while the kernel runs.  Called by two
// whole waves (tid = 0..127); false = the launch is being aborted.
template <bool OV>
__device__ __forceinline__ void s2_load_top(S2Side& sd, const FillParams& p, int s, int tid) {
    const int64_t jt = (int64_t)s * s2_stride<OV>() + tid;
    const bool want = tid < 127 && jt <= p.cols;
    int tv = 0;
    if (p.top_gran) {
        u64 gr = 0;
        uint64_t t0 = 0;
        unsigned n = 0;
        for (;;) {
            if (want) gr = __hip_atomic_load((gu64*)(p.top_gran + jt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const bool ok = !want || (u32)(gr >> 32) == p.top_tag;
            if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
            __builtin_amdgcn_s_sleep(8);
            if ((++n & 63u) == 0) {
                const uint64_t now = __builtin_amdgcn_s_memrealtime();
                if (t0 == 0) t0 = now;
                if (((now - t0) >> 10) > (uint64_t)p.top_wait_ticks)
                    __hip_atomic_store((gu32*)p.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load((gu32*)p.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) break;
            }
        }
        tv = (int)(u32)gr;
    } else if (p.top && want) {
        tv = p.top[jt];
    }
    sd.topv[tid] = tv;
}

// One importer wave of strip s: polls the self-tagged edge column of strip s - 1 in edge4 and feeds the LDS halo ring.
// false = abort.
// Pacing of a filler behind scouts (see the kernel): the importer hands the halo to the producer no faster than `inv` steps per
// 100 MHz tick from tick `start` on.  Calibrated by the importer itself when the first edge value of its scout arrives: that moment
// divided by the strip index is what a hand-off takes on THIS device in THIS launch.
struct S2Pace {
    bool on = false, set = false;
    int S = 0, s = 0, steps = 0, bps = 0;  // strips, my strip, steps of a strip, bytes a strip stores per step
    float inv = 0.f, start = 0.f;          // the line: step <= 64 + (tick - start) * inv
    // (everything else is read from the launch parameters when the line is drawn: the kernel has no registers to keep floats around)
    __device__ __forceinline__ void calibrate(const FillParams& p, float t_first) {
        int tau_ps = p.filler_tau_ps, hop_ps = p.filler_hop_ps, bw_gbs = p.filler_bw_gbs;
        asm volatile("" : "+s"(tau_ps), "+s"(hop_ps), "+s"(bw_gbs));   // (computed here, once: not hoisted out of the loops and kept in registers)
        const float tau_min = (float)tau_ps * 1e-4f, hop_host = (float)hop_ps * 1e-4f;   // ticks of 10 ns
        const float bw_per_tick = (float)bw_gbs * 10.f, fsteps = (float)steps;
        const float hop = (s >= 8) ? fminf(fmaxf(t_first / (float)s, 0.5f * hop_host), 1.5f * hop_host) : hop_host;
        start = (s >= 8) ? t_first : (float)s * hop;
        // every filler ends when the last one can at best: after all hand-offs plus one unhindered strip -- or, where the stores of
        // all strips together are the limit, when the shared bandwidth allows (rates steps / (D - s hop) summed over the strips <= B)
        // (split strips: the filler that ends last runs only p.filler_end_steps; the bytes all strips store are those of whole strips)
        const float esteps = p.filler_end_steps > 0 ? (float)p.filler_end_steps : fsteps;
        const float wsteps = p.filler_full_steps > 0 ? (float)p.filler_full_steps : fsteps;
        const float d_chain = (float)(S - 1) * hop + esteps * tau_min;
        const float x = bw_per_tick * hop / ((float)max(bps, 1) * wsteps);
        const float d_bw = (x < 20.f) ? (float)S * hop / (1.f - __expf(-x)) : 0.f;
        const float d = fmaxf(d_chain, d_bw);
        inv = (d > start + 1.f) ? fsteps / (d - start) : 0.f;
        set = true;
    }
};
// stop_u: leave once the halo is fed up to that step (the consumer waves of a scout that fills import until their blocks come up)
template <bool OV>
__device__ __forceinline__ bool s2_importer(S2Side& sd, const FillParams& p, int s_real, int phi, int UT, int rows, int gb, int ngap, int lane, bool synth = false,
                                            S2Pace pace = S2Pace(), int stop_u = 0x7fffffff) {
    const int s = synth ? 0 : s_real;   // (synth: timing experiments -- every strip invents its halo like strip 0)
    __builtin_amdgcn_s_setprio(2);
    const u32 row0v = (u32)(gb + sd.topv[0] + ngap * s_real * s2_stride<OV>());
    const int xl = s2_xlane<OV>();          // my step u needs the left strip's lane xl at ITS step u + xl + 1 (edge4 is indexed by step - 1)
    const int ulast = min(UT + 64, stop_u);
    const u32 tag = (u32)gb >> 24;
    const u32* e4 = (s > 0) ? p.edge4 + (int64_t)(s - 1) * p.e4stride : nullptr;
    int impu = 1;
    bool wide = true;
    // (polls of 16 / 32 values instead of 64 were measured worse: 16384^2 chain done after 1124 / 687 us against 653)
    Spin spin; spin.code = 3;
    const uint64_t pace_t0 = __builtin_amdgcn_s_memrealtime();
    while (impu <= ulast) {
        const int front = lds_load(&sd.halo_ready);
        if (front > 1) impu = max(impu, front);
        if (impu > ulast) break;
        int lim = min(ulast + 1, lds_load(&sd.prod_u) + SY_RH / 2 - 2 * SY_U);
        if (pace.set && pace.inv > 0.f) lim = min(lim, 64 + max(0, (int)(((float)(uint32_t)(__builtin_amdgcn_s_memrealtime() - pace_t0) - pace.start) * pace.inv)));
        int base = impu;
        auto windows = [&](auto NB) {
            constexpr int nbat = decltype(NB)::value;
            u32 vals[nbat];
            bool oks[nbat];
#pragma unroll
            for (int b4 = 0; b4 < nbat; ++b4) {
                const int u = impu + b4 * 64 + lane;
                const int r = u - phi;
                u32 v = row0v;
                bool ok = true;
                if (r > rows) v = (u32)gb;
                else if (r > 0) {
                    if (s == 0) v = (u32)(gb + ngap * r + (p.tile_left ? p.tile_left[(int64_t)r * p.M] : 0));   // (a column tile: the previous tile's last column, from H)
                    else {
                        v = __hip_atomic_load((gu32*)(e4 + u + xl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = (v >> 24) == tag;
                    }
                }
                vals[b4] = v;
                oks[b4] = ok && (u < lim);
            }
            const int front2 = lds_load(&sd.halo_ready);
#pragma unroll
            for (int b4 = 0; b4 < nbat; ++b4) {
                const int u = impu + b4 * 64 + lane;
                const u64 okm = __ballot(oks[b4]);
                const int npre = (okm == ~0ull) ? 64 : __builtin_ctzll(~okm);
                if (base == impu + b4 * 64 && npre > 0) {
                    if (lane < npre && (front2 <= 1 || u >= front2)) {
                        __hip_atomic_store(&sd.halo[(u - 1) & (SY_RH - 1)], vals[b4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(&sd.halo[(u - 1 + SY_RH / 2) & (SY_RH - 1)], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    base += npre;
                }
            }
        };
        if (wide) windows(std::integral_constant<int, 4>{});
        else windows(std::integral_constant<int, 1>{});
        wide = (base - impu) >= 64;
        if (base > impu) {
            asm volatile("" ::: "memory");
            if (pace.on && !pace.set && base > phi + 1)   // (the first phi steps lie above the matrix: nothing of the scout's is in them)
                pace.calibrate(p, (float)(uint32_t)(__builtin_amdgcn_s_memrealtime() - pace_t0));
            impu = base;
            __hip_atomic_fetch_max(&sd.halo_ready, impu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (spin.fail(p.abort_flag)) {
            return false;
        }
    }
    __builtin_amdgcn_s_setprio(0);
    return true;
}

// The producer wave of strip s: score profiles and start values of its lanes, then the strip loop -- producer_perm2 (LDS rings for
// the consumers of the same workgroup) or, for a scout, producer_scout2 (nothing but the edge column).  `exports`: lane 63 stores its
// B column to edge4.  Returns the asm loop's status (non-zero: a halo wait gave up).
template <bool SCOUT, bool LOCAL, bool OV>
__device__ __forceinline__ int s2_produce(S2Side& sd, Sys2Lds* full, const FillParams& p, const unsigned char* seq_a, const unsigned char* ltab,
                                          const unsigned char* bcode, int s, int S, int phi, int UT, int lane, int gb, int ngap, int mm, int xm, bool exports,
                                          bool local_rt = false, bool stamps_as_scout = false, int ua = -1) {
    const int jA = s * s2_stride<OV>() + 2 * lane - 1, jB = jA + 1;      // (cols < 2^20)
    const int topA = lane >= 1 ? sd.topv[2 * lane - 1] : 0, topB = sd.topv[2 * lane];
    // profiles: scores of the NEXT lane's A column and of my B column against the letter codes (7: outside the sequences)
    const int jn = jA + 2;
    const u32 ca = (lane < 63 && jn >= 1 && jn <= p.cols) ? (u32)ltab[seq_a[jn - 1]] : 8u;   // (ltab: the code table the prologue left in LDS)
    const u32 cb = (lane >= 1 && jB <= p.cols) ? (u32)ltab[seq_a[jB - 1]] : 8u;
    u32 palo = 0, pahi = 0, pblo = 0, pbhi = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        palo |= ((u32)(unsigned char)(signed char)((u32)c == ca ? mm : xm)) << (8 * c);
        pblo |= ((u32)(unsigned char)(signed char)((u32)c == cb ? mm : xm)) << (8 * c);
    }
#pragma unroll
    for (int c = 4; c < 7; ++c) {
        pahi |= ((u32)(unsigned char)(signed char)((u32)c == ca ? mm : xm)) << (8 * (c - 4));
        pbhi |= ((u32)(unsigned char)(signed char)((u32)c == cb ? mm : xm)) << (8 * (c - 4));
    }
    pahi |= ((u32)(unsigned char)(signed char)SW_PERM_PAD) << 24;
    pbhi |= ((u32)(unsigned char)(signed char)SW_PERM_PAD) << 24;
    if (lane == 0) {   // lane 0 has no columns of its own: its tA must stay below the halo values whatever the scores are
        const u32 pad4 = 0x01010101u * (u32)(unsigned char)(signed char)SW_PERM_PAD;
        pblo = pad4; pbhi = pad4;
    }
    // row-0 values: G(0, j) = bias + H(0, j) + ngap * j (H(0, j) = 0 unless a band has a row above); lane 0's A never changes
    // (the bias: below every G)
    const u32 ga1 = lane == 0 ? (u32)gb : (u32)(gb + topA + ngap * (int)jA), gb1 = (u32)(gb + topB + ngap * (int)jB);
    // floor of my A cell at local step 1 (the first step adds ngap before use)
    const u32 z0 = (u32)(gb + ngap * (1 - phi - lane + (int)jA));
    // A' stream: lane l, step u scores row u - phi - l, i.e. b[u - phi - l - 1]; the B stream is one row further
    const unsigned char* cbase = bcode + (p.bfront - phi - 64);   // (bcode: this workgroup's own copy of the letter codes of b)
    const u32 expoff = (exports && s + 1 < S && lane == s2_xlane<OV>()) ? 0u : SY_OOB;
    const uint64_t eb = (uint64_t)(uintptr_t)(p.edge4 + (int64_t)s * p.e4stride);
    const sw_i32x4p erc = {(int)(u32)eb, (int)(u32)(eb >> 32), 0x7FFFFF00, 0x00020000};
    int polls[2];
    // debug stamps: [2s, 2s+1] start / end of the strip (100 MHz), [4n+16+2s ..] slow-path polls; a filler behind scouts writes the
    // same at offset 6n + 32; [6n+16, 6n+17]: s_memtime around strip 0 (shader clock = d(memtime) / d(memrealtime) x 100 MHz)
    u64* const dbg = p.dbg ? p.dbg + ((!SCOUT && p.nscout > 0 && !stamps_as_scout) ? 6 * p.nstrips + 32 : 0) : nullptr;   // (a scout that fills stamps as the scout it is)
    if (dbg && lane == 0) {
        dbg[2 * s] = __builtin_amdgcn_s_memrealtime();
        if (s == 0 && dbg == p.dbg) p.dbg[6 * p.nstrips + 16] = __builtin_amdgcn_s_memtime();
        if (s == 0 && dbg == p.dbg) p.dbg[8 * p.nstrips + 32 + 3] = dbg[0];   // (S2_STAMP_FIRST_STEP, declared with the prologue below)
    }
    int st;
    if constexpr (SCOUT) {
        if constexpr (LOCAL) {   // (the reader of this strip's edge column runs on this XCD: the stores stay in its L2)
            st = producer_scout2_local(palo, pahi, pblo, pbhi, (u32)ngap, 63u - (u32)lane, z0, ga1, gb1, ga1 + (u32)SW_PERM_PAD, gb1 + (u32)SW_PERM_PAD, expoff, cbase,
                                       (u32)(size_t)&sd.halo[0], (u32)(size_t)&sd.lowv[0], (u32)(size_t)&sd.prod_u, UT, erc, polls);
        } else
            st = producer_scout2(palo, pahi, pblo, pbhi, (u32)ngap, 63u - (u32)lane, z0, ga1, gb1, ga1 + (u32)SW_PERM_PAD, gb1 + (u32)SW_PERM_PAD, expoff, cbase,
                                 (u32)(size_t)&sd.halo[0], (u32)(size_t)&sd.lowv[0], (u32)(size_t)&sd.prod_u, UT, erc, polls);
    } else {
        const u32 wA = (u32)(size_t)&full->ringA[0] + (u32)lane * (u32)SY_LSTR, wB = (u32)(size_t)&full->ringB[0] + (u32)lane * (u32)SY_LSTR;
        const int kc = 30 - SY_R - phi, kr = -SY_R - phi - 32;
        // lane 63's edge store exists twice, written through (" sc1") and kept in this XCD's L2 (" sc0"): one of the two has its offset out
        // of bounds (a dropped store costs the producer nothing measurable; two copies of the loop cost registers the kernel does not have)
        if (ua >= 0)   // a scout that fills: the scout's loop up to step ua, the filler's from there (sw_scoutfill_producer.inc)
            st = producer_scoutfill2(palo, pahi, pblo, pbhi, (u32)ngap, wA, wB, 63u - (u32)lane, z0, ga1, gb1, ga1 + (u32)SW_PERM_PAD, gb1 + (u32)SW_PERM_PAD,
                                     local_rt ? SY_OOB : expoff, local_rt ? expoff : SY_OOB, cbase, (u32)(size_t)&sd.halo[0], (u32)(size_t)&sd.lowv[0],
                                     (u32)(size_t)&full->cons_blk[0], (u32)(size_t)&sd.never, (u32)(size_t)&sd.prod_u, ua, UT, kc, kr, erc, polls);
        else
        st = producer_perm2(palo, pahi, pblo, pbhi, (u32)ngap, wA, wB, 63u - (u32)lane, z0, ga1, gb1, ga1 + (u32)SW_PERM_PAD, gb1 + (u32)SW_PERM_PAD,
                            local_rt ? SY_OOB : expoff, local_rt ? expoff : SY_OOB, cbase, (u32)(size_t)&sd.halo[0], (u32)(size_t)&sd.lowv[0],
                            (u32)(size_t)&full->cons_blk[0], (u32)(size_t)&sd.never, (u32)(size_t)&sd.prod_u, UT, kc, kr, erc, polls);
    }
    if (dbg && lane == 0) {   // strip times, then the slow-path polls (back-pressure / halo not there yet)
        dbg[2 * s + 1] = __builtin_amdgcn_s_memrealtime();
        if (s == 0 && dbg == p.dbg) p.dbg[6 * p.nstrips + 17] = __builtin_amdgcn_s_memtime();
        if (dbg == p.dbg) {
            dbg[4 * p.nstrips + 16 + 2 * s] = (u64)polls[0];
            dbg[4 * p.nstrips + 17 + 2 * s] = (u64)polls[1];
        }
    }
    return st;
}

// xcd_mode: the strips of XCD x -- fillers f0 .. f0 + nf - 1, scouts s0 .. s0 + ns - 1 in w workgroups, the first ndx of them with two strips
struct XcdLayout { int f0, nf, s0, ns, ndx, w; };
__device__ __forceinline__ XcdLayout xcd_layout(int S, int x, int extra = 0) {
    const int base = S >> 3, rem = S & 7;
    XcdLayout l;
    l.nf = base + (x < rem ? 1 : 0);
    l.f0 = x * base + min(x, rem);
    l.s0 = x ? l.f0 - 1 : 0;                 // (strip S - 1 has no scout: nobody reads its edge -- unless `extra`: split strips, below)
    l.ns = (x ? l.nf : l.nf - 1) + (x == 7 ? extra : 0);
    l.ndx = max(0, l.ns - (32 - l.nf));
    l.w = l.ns - l.ndx;
    return l;
}
// split strips: does strip t have a scout workgroup of its own (one strip, not two)?  Only such a scout can take over rows of its strip.
__device__ __forceinline__ bool strip_has_single_scout(int S, int t, int extra) {
    for (int x = 0; x < 8; ++x) {
        const XcdLayout l = xcd_layout(S, x, extra);
        if (t >= l.s0 && t < l.s0 + l.ns && t <= S - 2 + extra) return t - l.s0 >= 2 * l.ndx;
    }
    return false;
}
// Do the two readers of strip s's edge column -- the scout and the filler of strip s + 1 -- run on the XCD `my_xcc`?  Every workgroup
// of the launch has written its XCD (+ 1) to xtab[blockIdx.x] on its way in; waits for the two entries (false: launch aborted).
// And does the XCD's last scout (block `far_block`) run here too?  It is the one that writes this XCD's dirty edge lines back when the
// chain has passed (the kernel): without it nothing may be left in this L2.
__device__ __forceinline__ bool xcd_local_readers(const FillParams& p, int S, int s, unsigned my_xcc, int far_block, Spin& spin, bool& local) {
    const u32* xtab = (const u32*)(p.atab + SW_XTAB_OFF);
    int blocks[3] = {-1, -1, far_block};
    for (int x = 0; x < 8; ++x) {
        const XcdLayout l = xcd_layout(S, x, p.split_extra);
        const int t = s + 1;
        if (t >= l.f0 && t < l.f0 + l.nf) blocks[0] = 8 * (l.w + t - l.f0) + x;
        if (t <= S - 2 + p.split_extra && t >= l.s0 && t < l.s0 + l.ns) blocks[1] = 8 * ((t - l.s0 < 2 * l.ndx) ? (t - l.s0) / 2 : t - l.s0 - l.ndx) + x;
    }
    local = true;
    for (int i = 0; i < 3; ++i) {
        if (blocks[i] < 0) continue;
        u32 v;
        while ((v = __hip_atomic_load((gu32*)(xtab + blocks[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u)
            if (spin.fail(p.abort_flag)) return false;
        local = local && v == my_xcc + 1u;
    }
    return true;
}

// ---- ONE launch per fill (round 4).  What a fill needs before its first step -- which letters occur (the code table), the padded
// copy of b and its letter codes, zeros in row 0 / column 0 of the matrices -- used to be two kernels in front of this one
// (sw_prep_scan, sw_prep_code), and the result was written by a third behind it (sw_finalize): ~9 us of dispatch each around a 0.8 ms
// fill.  Now every workgroup does its share on the way in and the last workgroup to leave writes the result:
//   prologue  scan 1/G of the letters -> OR into the launch's presence map (8 agent-scope atomics) -> ONE grid barrier (the G
//             workgroups of a launch are resident together anyway: they wait for each other's edge columns) -> code table in LDS ->
//             the workgroup's OWN padded copy of b and of its codes (read by its producer / consumers only: no second barrier, nothing
//             shared across the XCDs' L2s inside the kernel) -> 1/G of row 0 / column 0;
//   epilogue  every wave waits for its own atomics, the workgroup counts itself out; the last one converts the arg-max key into the
//             sw_result and re-arms key, abort flag, XCD table and the sync words for the next launch (they are zero between launches).
// More than 7 letters: nothing is filled here -- workgroup 0 leaves the shared padded copies for sw_systolic, which is enqueued right
// behind and checks the letter count for itself (and then runs this same epilogue).
struct S2Prep {
    __attribute__((aligned(16))) unsigned char tab[256];
    unsigned int pres[8];
    int nletters, ok;
};
constexpr int S2_SYNC_BAR = 0, S2_SYNC_OUT = 1, S2_SYNC_MAP = 8;

// debug stamps of the launch's own overhead (debug_buf), 100 MHz ticks, in slots of their own behind everything the strips stamp:
// dbg[8 n + 32 + k] for n = p.nstrips --  0: workgroup 0 enters;  1: the last workgroup knows the alphabet (past the grid barrier, or done
// with its own scan);  2: the last workgroup leaves the prologue;  6: the last workgroup enters;  3: strip 0's producer takes its first step;  4: the last wave has its
// stores acknowledged;  5: the last workgroup out has re-armed the launch words.  (1, 2, 4, 6: maxima over the launch -- the buffer starts zeroed)
enum { S2_STAMP_ENTRY = 0, S2_STAMP_ALPHABET = 1, S2_STAMP_PROLOGUE = 2, S2_STAMP_FIRST_STEP = 3, S2_STAMP_STORES = 4, S2_STAMP_OUT = 5, S2_STAMP_LAST_ENTRY = 6 };
__device__ __forceinline__ void s2_stamp(const FillParams& p, int k, bool is_max) {
    u64* const slot = p.dbg + 8 * p.nstrips + 32 + k;
    const u64 now = __builtin_amdgcn_s_memrealtime();
    if (is_max) (void)__hip_atomic_fetch_max(slot, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *slot = now;
}

// The letters of seq[0 .. n) into the workgroup's presence map, 16 bytes per thread and load, four loads in flight (the loads are
// aligned: what they read beyond either end of the sequence lies in the same 16 bytes as a byte of it, and is masked out).  A thread
// keeps the map word it looked at last in a register, with the bits it has seen there: a letter costs an LDS access only when its word
// changes or its bit is new -- with the few letters of a real sequence, once per thread.  (Bound by VALU issue, ~15 instructions per
// byte: 32 K letters take ~9 us, as they did with a lookup in LDS for every byte; DESIGN.md section 6.)
__device__ __forceinline__ void s2_scan_all(S2Prep& pp, const unsigned char* __restrict__ seq, int64_t n, int tid, int nth) {
    if (n <= 0) return;
    const uintptr_t a0 = (uintptr_t)seq & ~(uintptr_t)15;
    const int64_t skew = (int64_t)((uintptr_t)seq - a0), nchunk = (skew + n + 15) >> 4;
    u32 cw = 8u, cm = 0u;   // (no word yet)
    for (int64_t c0 = tid; c0 < nchunk; c0 += 4 * (int64_t)nth) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t c = c0 + (int64_t)u * nth;
            v[u] = c < nchunk ? *(const uint4*)(a0 + 16 * (uintptr_t)c) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t c = c0 + (int64_t)u * nth;
            if (c >= nchunk) break;
            const u32 w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            const int64_t first = skew - 16 * c, end = skew + n - 16 * c;   // bytes [first, end) of the chunk belong to the sequence
            const bool whole = first <= 0 && end >= 16;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (!whole && (q < first || q >= end)) continue;
                const u32 ch = (w[q >> 2] >> (8 * (q & 3))) & 255u;
                const u32 bit = 1u << (ch & 31u);
                if ((ch >> 5) != cw) { cw = ch >> 5; cm = __hip_atomic_load(&pp.pres[cw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
                if (!(cm & bit)) { atomicOr(&pp.pres[cw], bit); cm |= bit; }
            }
        }
    }
}

__device__ __forceinline__ int s2_prologue(S2Prep& pp, const FillParams& p, const unsigned char* __restrict__ seq_a, const unsigned char* __restrict__ seq_b) {
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x, G = (int)gridDim.x, wg = (int)blockIdx.x;
    gu32* const sync = (gu32*)p.sync;
    if (p.dbg && wg == 0 && tid == 0) s2_stamp(p, S2_STAMP_ENTRY, false);
    if (p.dbg && tid == 0) s2_stamp(p, S2_STAMP_LAST_ENTRY, true);
    if (tid < 8) pp.pres[tid] = 0u;
    if (tid == 0) pp.ok = 1;
    __syncthreads();
    if (p.scan_all) {
        // (1+2) every workgroup scans all the letters for itself: nothing shared, nobody to wait for.  (a column tile scans the whole a:
        // every tile must decide alike -- and so must every workgroup: all of them read the same bytes)
        s2_scan_all(pp, p.alpha_a, p.alpha_cols, tid, nth);
        s2_scan_all(pp, seq_b, p.rows, tid, nth);
    } else {
        {   // (1) my 1/G of the letters
            const int64_t acols = p.alpha_cols, total = acols + p.rows, chunk = (total + G - 1) / G;   // (a column tile scans the whole a: every tile must decide alike)
            const int64_t lo = (int64_t)wg * chunk, hi = min(total, lo + chunk);
            for (int64_t i = lo + tid; i < hi; i += nth) {
                const unsigned char ch = i < acols ? p.alpha_a[i] : seq_b[i - acols];
                atomicOr(&pp.pres[ch >> 5], 1u << (ch & 31));
            }
        }
        __syncthreads();
        if (tid < 64) {   // (2) wave 0: publish, arrive, wait for everybody, fetch the launch's map
            if (tid < 8 && pp.pres[tid]) (void)__hip_atomic_fetch_or(sync + S2_SYNC_MAP + tid, pp.pres[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // (the wave's atomics are performed before its arrival counts)
            if (tid == 0) (void)__hip_atomic_fetch_add(sync + S2_SYNC_BAR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            Spin spin; spin.code = 17;
            bool ok = true;
            while ((u32)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(sync + S2_SYNC_BAR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < (u32)G)
                if (spin.fail(p.abort_flag)) { ok = false; break; }
            if (tid < 8) pp.pres[tid] = __hip_atomic_load(sync + S2_SYNC_MAP + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tid == 0) pp.ok = ok ? 1 : 0;
        }
    }
    __syncthreads();
    if (p.dbg && tid == 0) s2_stamp(p, S2_STAMP_ALPHABET, true);
    if (!pp.ok) return -1;
    if (tid < 256) {   // (3) code of a byte value = its rank among the values present (7 = not a letter / too many letters)
        int rank = 0, nl = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const unsigned int m = pp.pres[w];
            nl += __popc(m);
            if (w < (tid >> 5)) rank += __popc(m);
            else if (w == (tid >> 5)) rank += __popc(m & ((1u << (tid & 31)) - 1u));
        }
        const bool here = (pp.pres[tid >> 5] >> (tid & 31)) & 1u;
        pp.tab[tid] = (here && nl <= 7) ? (unsigned char)rank : (unsigned char)7;
        if (tid == 0) pp.nletters = nl;
    }
    __syncthreads();
    const int nl = pp.nletters;
    const int64_t per = p.bpad_pstride, front = p.bfront, rows = p.rows;
    if (wg == 0) {   // for the fall-back kernel (and sw_get_option): the table and the letter count
        if (tid < 256) p.atab_w[tid] = pp.tab[tid];
        if (tid == 0) *(unsigned int*)(p.atab_w + 256) = (unsigned int)nl;
        if (nl > 7)   // ... and the shared padded copies it reads (sw_prep_code's layout)
            for (int64_t i = tid; i < per; i += nth) {
                const bool in = (i >= front && i - front < rows);
                const unsigned char ch = in ? seq_b[i - front] : (unsigned char)0;
                p.bpad8_w[i] = ch;
                p.bpad16_w[i] = in ? (unsigned short)ch : (unsigned short)0x100;
                p.bcode_w[i] = (unsigned char)7;
            }
    }
    if (nl <= 7) {
        // (4) my own [bpad8 | bcode]: 16 bytes per thread and pass (per and front are multiples of 16, seq_b and the copies are 16-byte
        // aligned): a 16384-row b is two passes of the workgroup, where 4 bytes per thread made six, one memory latency each
        unsigned char* const mine = p.priv + (int64_t)wg * p.priv_stride;
        for (int64_t i = 16 * (int64_t)tid; i < per; i += 16 * (int64_t)nth) {
            const int64_t k = i - front;
            u32 raw[4] = {0u, 0u, 0u, 0u}, code[4] = {0x07070707u, 0x07070707u, 0x07070707u, 0x07070707u};
            if (k >= 0 && k + 16 <= rows) {
                const uint4 v = *(const uint4*)(seq_b + k);
                raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w;
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    code[d] = (u32)pp.tab[raw[d] & 255u] | ((u32)pp.tab[(raw[d] >> 8) & 255u] << 8) | ((u32)pp.tab[(raw[d] >> 16) & 255u] << 16) | ((u32)pp.tab[raw[d] >> 24] << 24);
            } else if (k + 16 > 0 && k < rows) {
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (k + q >= 0 && k + q < rows) {
                        const u32 ch = seq_b[k + q];
                        raw[q >> 2] |= ch << (8 * (q & 3));
                        code[q >> 2] = (code[q >> 2] & ~(0xffu << (8 * (q & 3)))) | ((u32)pp.tab[ch] << (8 * (q & 3)));
                    }
            }
            *(uint4*)(mine + i) = make_uint4(raw[0], raw[1], raw[2], raw[3]);
            *(uint4*)(mine + per + i) = make_uint4(code[0], code[1], code[2], code[3]);
        }
        // (5) my 1/G of [row 0 | column 0] of the matrices (a band's row 0 is its halo row: H comes from the kernel, P belongs to the band above)
        // (a column tile behind another one: its column 0 is that tile's last column)
        const int64_t M = p.M, nrow0 = p.cols + 1, nedge = nrow0 + rows, chunk = (nedge + G - 1) / G;
        const int64_t lo = (int64_t)wg * chunk, hi = min(nedge, lo + chunk);
        void* const H = p.H; void* const P = (void*)p.P;
        const bool own_col0 = p.tile_left == nullptr;
        for (int64_t e = lo + tid; e < hi; e += nth) {
            if (e < nrow0) {
                if (!p.skip_row0 && (e > 0 || own_col0)) {
                    if (H) { if (p.h_bytes == 8) ((int64_t*)H)[e] = 0; else ((int32_t*)H)[e] = 0; }
                    if (P) { if (p.p_bytes == 1) ((signed char*)P)[e] = 0; else ((int32_t*)P)[e] = 0; }
                }
            } else if (own_col0) {
                const int64_t r = e - nrow0 + 1;
                if (H) { if (p.h_bytes == 8) ((int64_t*)H)[r * M] = 0; else ((int32_t*)H)[r * M] = 0; }
                if (P) { if (p.p_bytes == 1) ((signed char*)P)[r * M] = 0; else ((int32_t*)P)[r * M] = 0; }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // my copies are in the L2 before any wave of this workgroup reads them
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (p.dbg && tid == 0) s2_stamp(p, S2_STAMP_PROLOGUE, true);
    return nl;
}

// worked: this launch was the one to fill (or was aborted): report and re-arm; otherwise only the sync words are reset
__device__ __forceinline__ void s2_epilogue(const FillParams& p, bool worked) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's arg-max atomics (and stores) are acknowledged
    if (p.dbg && (threadIdx.x & 63u) == 0) s2_stamp(p, S2_STAMP_STORES, true);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    // wave 0: lane 0 counts the workgroup out; the last workgroup's whole wave re-arms (the XCD table is 256 words: four stores per lane
    // where one thread issued 256 in a row)
    const int lane = (int)threadIdx.x;
    gu32* const sync = (gu32*)p.sync;
    u32 prev = 0u;
    if (lane == 0) prev = __hip_atomic_fetch_add(sync + S2_SYNC_OUT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((u32)__builtin_amdgcn_readfirstlane((int)prev) != gridDim.x - 1u) return;
    // the last workgroup out (a column tile that is not the matrix' last one leaves key and abort flag to the tiles behind it)
    if (lane == 0 && worked && p.final_launch) {
        const u64 k = __hip_atomic_load((gu64*)p.result_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u32 ab = __hip_atomic_load((gu32*)p.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p.result) {
            p.result->max_score = (int64_t)(k >> 40);
            p.result->max_pos = k ? (int64_t)(SW_KEY_IDX_MASK - (k & SW_KEY_IDX_MASK)) : 0;
            p.result->path_len = ab ? -(int64_t)ab : 0;   // (< 0: a hand-off wait gave up; the value says which kind)
        }
        __hip_atomic_store((gu64*)p.result_key, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store((gu32*)p.abort_flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (worked) {
        gu32* const xtab = (gu32*)(p.atab_w + SW_XTAB_OFF);
#pragma unroll
        for (int i = 0; i < 256; i += 64) __hip_atomic_store(xtab + i + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane < 8) __hip_atomic_store(sync + S2_SYNC_MAP + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) {
        __hip_atomic_store(sync + S2_SYNC_BAR, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sync + S2_SYNC_OUT, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p.dbg) s2_stamp(p, S2_STAMP_OUT, false);
    }
}

template <int NC, bool OV>
__device__ __forceinline__ void s2_body(Sys2Lds& lds, const unsigned char* ltab, const unsigned char* my_bpad8, const unsigned char* my_bcode,
                                        const unsigned char* seq_a, const FillParams& p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t M = p.M;
    const int rows = (int)p.rows;
    const int ngap = p.ngap, mm = p.mm, xm = p.xm;
    const int S = p.nstrips;                     // ceil(cols / 126)
    const int gb = (int)p.gbias;
    const int nscout = p.nscout;                 // workgroups 0 .. nscout-1 are scouts (0: none -- the strips chain through each other)

    // ---- role of this workgroup: scout of sc_cnt strips from sc_s0 on, or filler of the strips fill_s, fill_s + fill_step, ...
    int sc_cnt = 0, sc_s0 = 0, sc_far = -1, sc_far_block = -1, fill_s = S, fill_step = S;
    unsigned my_xcc = 0;
    if (p.xcd_mode == 1) {
        // Workgroup i runs on XCD i % 8 (seen by the host's sw_xcc_probe; a scout still asks where its readers really are before it
        // keeps anything in its L2: xcd_local_readers below).  XCD x gets the fillers of the
        // strips f0 .. f0 + nf - 1 (an eighth of them) and the scouts of f0 - 1 .. f0 + nf - 2: a scout's edge column is read by the
        // scout and by the filler of the NEXT strip, which then sit on its own XCD -- all but the XCD's last scout keep their edge
        // stores in the XCD's L2 (" sc0"; sw_scout_producer.inc).  32 workgroups per XCD, one per CU: where fillers + scouts are
        // more than that, the first scout workgroups carry two strips.
        const int x = (int)blockIdx.x & 7, k = (int)blockIdx.x >> 3;
        const XcdLayout l = xcd_layout(S, x, p.split_extra);
        const int nf = l.nf, f0 = l.f0, s0 = l.s0, ns = l.ns, ndx = l.ndx, w = l.w;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
        my_xcc &= 15u;
        if (threadIdx.x == 0) __hip_atomic_store((gu32*)(p.atab + SW_XTAB_OFF) + blockIdx.x, my_xcc + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k < w) {
            sc_cnt = k < ndx ? 2 : 1;
            sc_s0 = s0 + (k < ndx ? 2 * k : k + ndx);
            sc_far = s0 + ns - 1;                                    // its reader scout is on the next XCD
            sc_far_block = 8 * ((ns - 1 < 2 * ndx) ? (ns - 1) / 2 : ns - 1 - ndx) + x;
        } else if (k - w < nf) {
            fill_s = f0 + k - w;
        } else {
            return;
        }
    } else if (p.xcd_mode == 2) {
        // The classic chain (no scouts), dealt per XCD: the gridDim.x workgroups of a pass take their strips in the order
        // [workgroups of XCD 0 | of XCD 1 | ...] instead of by blockIdx, so that a strip's right-hand neighbour runs on the same XCD --
        // except across the seven seams -- and the producer keeps its edge stores in that XCD's L2 (" sc0") once it has seen that the
        // neighbour really is there.
        const int G = (int)gridDim.x, x = (int)blockIdx.x & 7, k = (int)blockIdx.x >> 3;
        int off = 0;
        for (int y = 0; y < x; ++y) off += (G - y + 7) >> 3;
        if (threadIdx.x == 0) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            __hip_atomic_store((gu32*)(p.atab + SW_XTAB_OFF) + blockIdx.x, (xcc & 15u) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        fill_s = off + k;
        fill_step = G;
    } else if ((int)blockIdx.x < nscout) {
        const int nd = p.scout_double, b = (int)blockIdx.x;
        sc_cnt = b < nd ? 2 : 1;
        sc_s0 = b < nd ? 2 * b : b + nd;
    } else {
        fill_s = (int)blockIdx.x - nscout;
        fill_step = (int)gridDim.x - nscout;
    }

    // ---- Split strips (round 4).  The fill ends  (S - 1) hand-offs + one strip at the FILLER's pace  after it began: a filler's producer
    // shares its CU with nine busy waves and needs 25 ns per row where a scout needs 20, and the last filler starts with the last scout.
    // But a scout's CU has room: from strip p.split_from on, a scout with a strip of its own also has consumer waves; they sleep until
    // block p.split_blk and write the strip's LOWER rows from there, while the strip's filler stops after the upper blocks.  The
    // producer of such a scout is the scout's loop down to the split and the filler's (rings, back-pressure) below it, in one asm
    // statement (sw_scoutfill_producer.inc) -- a filler-type producer from the first row on, with polling importers beside it, needed
    // 31 ns per row and made the fill 8 % SLOWER.  So the scout keeps its pace for the upper part and runs only the lower part at the
    // filler's; the filler is done after split_blk blocks: both end ~12 % earlier than a whole strip at the filler's pace.  (The last strip gets a scout for this, p.split_extra; scouts that carry two strips do not split.)
    const int split_blk = (p.xcd_mode == 1) ? p.split_blk : 0;
    bool sf = false;          // this workgroup is a scout that also fills (the lower blocks of strip fill_s)
    if (split_blk > 0 && sc_cnt == 1 && sc_s0 >= p.split_from) { sf = true; fill_s = sc_s0; fill_step = S; sc_cnt = 0; }
    else if (sc_cnt == 1 && sc_s0 == S - 1) return;   // (an extra scout of the last strip that has nothing to take over)

    if (sc_cnt) {
        // ---- scout workgroup: strips sc_s0 (and sc_s0 + 1).  SIMD class of a wave: wave & 3 (waves w, w+4, w+8 share a SIMD;
        // tools/ubench_hwid.hip).  Wave 0 is the producer of the first strip, alone on its SIMD (waves 4, 8 stay parked); with two strips
        // wave 1 is the producer of the second (5, 9 parked) and classes 2 / 3 hold the importers of the first / second strip.
        S2Side* sides = (S2Side*)&lds;
        const int cnt = sc_cnt, s0 = sc_s0;
        const int cls = wave & 3;
        // importers: with two strips ONE wave each -- every polling wave more slows both producers of the CU through the memory pipeline
        // (step 21.9 / 30.7 / 45 ns with 1 / 2 / 3 importers per strip); with one strip every wave off the producer's SIMD -- nine.  In
        // the per-XCD dealing (polls that hit the L2) the chain of 16384^2 ends after 640 us with six and 630 with nine against 655-660
        // with three (12288^2: 0.587 ms per fill against 0.602); with one or two it is as with three.  (debug bits 24-25: that many
        // importer waves on SIMD 2 only)
        const int nimp_dbg = (p.debug_flags >> DBG_S2_IMPORTERS_SHIFT) & 3;
        const bool producer = wave < cnt;
        const bool importer = !producer && (cnt == 2 ? (cls >= 2 && (wave >> 2) < (nimp_dbg ? nimp_dbg : 1))
                                                     : (nimp_dbg ? (cls == 2 && (wave >> 2) < nimp_dbg) : cls != 0));
        const int half = producer ? wave : (cnt == 2 ? cls - 2 : 0);
        if (threadIdx.x < 2) { sides[threadIdx.x].prod_u = 0; sides[threadIdx.x].halo_ready = 1; sides[threadIdx.x].never = 0x7fffffff; }
        for (int i = threadIdx.x; i < 2 * SY_RH; i += blockDim.x) sides[i / SY_RH].halo[i % SY_RH] = 0u;
        if (threadIdx.x < 256) sides[threadIdx.x >> 7].lowv[threadIdx.x & 127] = (u32)gb;
        if (threadIdx.x < 256 && (int)(threadIdx.x >> 7) < cnt && s0 + (int)(threadIdx.x >> 7) < S)
            s2_load_top<OV>(sides[threadIdx.x >> 7], p, s0 + (int)(threadIdx.x >> 7), (int)(threadIdx.x & 127));
        __syncthreads();
        if (p.top_gran && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load((gu32*)p.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) return;
        const int s = s0 + half;
        if (s < S && (producer || importer)) {
            const int phi = S - 1 - s;
            const int UT = ((rows + SY_U - 1) / SY_U * SY_U + 63 + phi + 63) / 64 * 64;   // (through the last 16-row block, also a short one)
            if (producer) {
                bool local = false;
                if (p.xcd_mode == 1 && s != sc_far && my_xcc == (blockIdx.x & 7u)) {
                    Spin spin; spin.code = 16;
                    if (!xcd_local_readers(p, S, s, my_xcc, sc_far_block, spin, local)) return;
                }
                const int st = local ? s2_produce<true, true, OV>(sides[half], nullptr, p, seq_a, ltab, my_bcode, s, S, phi, UT, lane, gb, ngap, mm, xm, !(p.debug_flags & DBG_S2_SCOUTS_NO_EXPORT))
                                     : s2_produce<true, false, OV>(sides[half], nullptr, p, seq_a, ltab, my_bcode, s, S, phi, UT, lane, gb, ngap, mm, xm, !(p.debug_flags & DBG_S2_SCOUTS_NO_EXPORT));
                if (st) __hip_atomic_store((gu32*)p.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // The XCD's last scout: the chain has passed, every edge column of this XCD's scouts sits dirty in its L2.  None of that may
                // outlive the launch there -- a later launch deals the strips differently, and a stale line written back after the new
                // owner's would hide that one's values from whoever reads memory.  An agent-scope release (buffer_wbl2 sc1) writes the
                // XCD's dirty lines back; once per XCD and launch (after every scout: 4 % of a 16384^2 fill).
                if (p.xcd_mode == 1 && s == sc_far) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            } else {
                (void)s2_importer<OV>(sides[half], p, s, phi, UT, rows, gb, ngap, lane, (p.debug_flags & DBG_S2_SYNTH_HALO) != 0);
            }
        }
        return;
    }

    int32_t* const H = (int32_t*)p.H;                 // may be NULL (not written); int64 elements when p.h_bytes == 8
    const bool h64 = p.h_bytes == 8;
    const int hsh = h64 ? 1 : 0;                      // H element index -> int32 index
    char* const P = (char*)p.P;                       // int32 or int8 codes, may be NULL
    const bool p8 = p.p_bytes == 1;
    const bool has_top = p.top != nullptr || p.top_gran != nullptr;
    S2Side& sd = lds.side;
    // role of each wave: wave 0 (SIMD 0, alone: waves 4 and 8 only take part in the barriers) is the producer; of the nine
    // others the first NC are consumers, the rest importers
    const int k9 = wave - 1 - (wave >> 2);        // ordinal among the waves off SIMD 0
    const bool off0 = (wave & 3) != 0;
    // (a scout that fills: its consumer waves are importers until the producer nears their first block -- a scout wants every wave polling for
    // its hand-off -- and then the full set of consumers: with four, the stores of the strip's lower blocks did not keep up with the producer)
    const int nc_eff = NC;
    const bool producer = wave == 0, consumer = off0 && k9 < nc_eff, importer = off0 && k9 >= nc_eff;

    for (int s = fill_s; s < S; s += fill_step) {
        // split strips: the blocks [q_lo, q_hi) of the strip are this workgroup's to write (a scout that fills: the lower ones; the filler of
        // such a strip: the upper ones, and its producer stops with them)
        const int nblk_all = (rows + SY_U - 1) / SY_U;
        const bool upper = split_blk > 0 && !sf && s >= p.split_from && strip_has_single_scout(S, s, p.split_extra);
        const int q_lo = sf ? min(split_blk, nblk_all) : 0, q_hi = upper ? min(split_blk, nblk_all) : nblk_all;
        if (threadIdx.x == 0) { sd.prod_u = 0; sd.halo_ready = 1; sd.never = 0x7fffffff; }
        if (threadIdx.x < 8) lds.cons_blk[threadIdx.x] = ((int)threadIdx.x < nc_eff) ? q_lo - 1 : 0x7fffffff;   // (blocks below q_lo count as consumed)
        for (int i = threadIdx.x; i < SY_RH; i += blockDim.x) sd.halo[i] = 0u;
        if (threadIdx.x < 128) sd.lowv[threadIdx.x] = (u32)gb;
        if (threadIdx.x < 128) s2_load_top<OV>(sd, p, s, (int)threadIdx.x);
        __syncthreads();
        if (p.top_gran && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load((gu32*)p.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) return;
        const int topA = lane >= 1 ? sd.topv[2 * lane - 1] : 0, topB = sd.topv[2 * lane];
        const int phi = S - 1 - s;
        const int UT = (q_hi * SY_U + 63 + phi + 63) / 64 * 64;   // (through the last 16-row block of this workgroup, also a short one)
        const int jA = s * s2_stride<OV>() + 2 * lane - 1, jB = jA + 1;      // (cols < 2^20)
        if (producer) {
            // (with scouts ahead the edge columns are theirs: a filler exports nothing)
            // classic chain per XCD: the workgroup that takes the strips to the right of mine in every pass (the next pass's first strip
            // follows this pass's last: its workgroup is on XCD 0, a seam) -- is it where the dealing put it, on my XCD?  Decided at the
            // first strip, kept in LDS (the kernel has no register to spare).
            bool local = false;
            if (p.xcd_mode == 2) {
                if (s == fill_s) {
                    unsigned xcc;
                    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                    xcc &= 15u;
                    const int x = (int)blockIdx.x & 7, k = (int)blockIdx.x >> 3, nx = ((int)gridDim.x - x + 7) >> 3;
                    int dec = 0;
                    if (k + 1 < nx && xcc == (unsigned)x) {
                        Spin spin; spin.code = 16;
                        u32 v;
                        while ((v = (u32)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load((gu32*)(p.atab + SW_XTAB_OFF) + 8 * (k + 1) + x, __ATOMIC_RELAXED,
                                                                                                __HIP_MEMORY_SCOPE_AGENT))) == 0u)
                            if (spin.fail(p.abort_flag)) return;
                        dec = (v == xcc + 1u) ? 1 : 0;
                    }
                    lds_store(&sd.pad, dec);
                }
                local = __builtin_amdgcn_readfirstlane(lds_load(&sd.pad)) == 1;
            }
            if (sf && s != sc_far && s + 1 < S && my_xcc == (blockIdx.x & 7u)) {   // (a scout that fills keeps its edge stores in this XCD's L2 like any scout)
                Spin spin; spin.code = 16;
                if (!xcd_local_readers(p, S, s, my_xcc, sc_far_block, spin, local)) return;
            }
            const int st = s2_produce<false, false, OV>(sd, &lds, p, seq_a, ltab, my_bcode, s, S, phi, UT, lane, gb, ngap, mm, xm, nscout == 0 || sf, local, sf,
                                             sf ? max(0, (q_lo * SY_U + phi - 1) / 64 * 64) : -1);
            if (st) {
                __hip_atomic_store((gu32*)p.abort_flag, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            if (sf && s == sc_far) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // (the XCD's last scout writes its L2's edge lines back: see the scouts)
            // (its edge column sits dirty in this XCD's L2: written back before anything of it could outlive the launch there -- see
            // the scouts' write-back above)
            if (local && s + fill_step >= S) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        } else if (consumer) {
            const int nblk = q_hi;   // (the matrix' last block may be short: its rows below the matrix are computed and dropped)
            const unsigned char* bchars = my_bpad8 + p.bfront;   // b, zero padded (the block's 16 characters are one scalar load)
            const u32* rA = (const u32*)&lds.ringA[lane * SY_LSTR];
            const u32* rB = (const u32*)&lds.ringB[lane * SY_LSTR];
            const bool okA = lane >= 1 && jA <= p.cols, okB = lane >= 1 && jB <= p.cols;
            const int aA = okA ? (int)seq_a[jA - 1] : SY_ASENT, aB = okB ? (int)seq_a[jB - 1] : SY_ASENT + 1;
            // one 8-byte store per matrix and row for the lanes that own two columns; with an odd number of columns the last
            // strip has one lane that owns only its A column
            const u32 voff2 = okB ? (u32)jA * 4u : SY_OOB, voff1 = (okA && !okB) ? (u32)jA * 4u : SY_OOB;
            const bool tail1 = (s == S - 1) && (p.cols & 1);
            const u32 rowb = (u32)(M * 4);
            int best = 0, bestrow = 0, bestcol = 0, bestq = -1;   // (the odd-column path below runs only for int32 H + P without a halo row)
            Spin spin; spin.code = 2;
            if (!tail1) {
                // the block in one asm statement.  With H in HBM the cell of the maximum is found at the end by re-reading the block
                // that held it; without H the block statement records it (2 * row-in-block + column)
                const u32 laneA = (u32)(size_t)rA, laneB = (u32)(size_t)rB;
                const u32 mm_v = (u32)mm, xm_v = (u32)xm, ngap_v = (u32)ngap;
                const u32 slot_addr = (u32)(size_t)&lds.cons_blk[k9];
                const u32 g0a = (u32)(gb + topA + ngap * (int)jA), g0b = (u32)(gb + topB + ngap * (int)jB);
                const bool nostore = (p.debug_flags & DBG_NO_STORES) != 0;   // timing experiments: drop the H / P stores
                const bool nt = p.store_nt != 0, store_h = H != nullptr && !nostore, store_p = P != nullptr && !nostore, trk = H == nullptr;
                const u32 voffH = (okB && store_h) ? (u32)jA * (h64 ? 8u : 4u) : SY_OOB, voffP = (okB && store_p) ? (u32)jA * (p8 ? 1u : 4u) : SY_OOB;
                const u32 rowbH = (u32)(M * (h64 ? 8 : 4)), rowbP = (u32)(M * (p8 ? 1 : 4));
                int bestcode = 0;
                constexpr int W = s2_stride<OV>();
                // whole-line stores (sw_wholeline_consumer.inc): overlapping strips, int32 P and H (int32 or int64) both written, laid out so that
                // the pairs of the odd matrix rows are 8-byte aligned (an odd row pitch, aligned matrices); the first and the last strip of the
                // launch have a neighbour missing and store every piece they have, as ever
                const bool allod = (M & 1) == 0;   // (an even row pitch: the pairs of every row sit at odd dwords, every row stores shifted pairs)
                const bool wlaunch = OV && H != nullptr && !(P != nullptr && p8 && (h64 || allod)) && !trk && !p.bot_gran && !has_top &&   // (P may be absent: its stores are dropped)
                                     ((uintptr_t)H & (h64 ? 15u : 7u)) == 0 && ((uintptr_t)P & 7u) == 0;
                const bool wl = wlaunch && s > 0 && s < S - 1;
                // whose cells are whose to report: a strip's own columns W s + 1 .. W s + W (the last strip: all it has); with whole-line stores
                // the cells a strip STORED (found when the maximum is looked up below)
                const bool mine = !OV || wlaunch || s == S - 1 || lane <= (W >> 1);
                // (row k of every block of a strip has the same alignment: which of the lane's pieces are this strip's to store, one bit per
                //  row and matrix -- set: not mine)
                u32 wm = 0;
                if (wl) {
                    const int64_t c1 = (int64_t)s * W + 1;
                    const u32 f0H = (u32)(((uint64_t)(uintptr_t)H + (uint64_t)(((M + c1) * 4) << hsh)) & 63u), f0P = (u32)(((uint64_t)(uintptr_t)P + (uint64_t)((M + c1) * 4)) & 63u);
                    const u32 pszH = h64 ? 16u : 8u, spanH = h64 ? 880u : 440u;
#pragma nounroll
                    for (int k = 0; k < SY_U; ++k) {   // (a real loop: unrolled, its 60 lane terms are hoisted out of the strip loop and spilled)
                        const bool odr = allod || (k & 1);
                        const u32 pcH = pszH * (u32)(lane - 1) - (odr ? pszH / 2 : 0u), pcP = 8u * (u32)(lane - 1) - (odr ? 4u : 0u);
                        if (!((u32)(pcH - ((f0H + (u32)k * rowbH + pcH) & 63u)) < spanH)) wm |= 1u << k;
                        if (!((u32)(pcP - ((f0P + (u32)k * rowbP + pcP) & 63u)) < 440u)) wm |= 1u << (16 + k);
                    }
                }
                if (has_top && store_h && k9 == 0 && p.skip_row0 != 2) {   // a band's row 0 is the halo row: H written, P left alone (a tile's: neither)
                    if (h64) {   // (scores are never negative: the high dword is zero)
                        if (okA) ((int64_t*)H)[jA] = topA;
                        if (okB) ((int64_t*)H)[jB] = topB;
                        if (s == 0 && lane == 0) ((int64_t*)H)[0] = topB;
                    } else {
                        if (okA) H[jA] = topA;
                        if (okB) H[jB] = topB;
                        if (s == 0 && lane == 0) H[0] = topB;
                    }
                }
                for (int q = q_lo + k9; q < nblk; q += nc_eff) {
                    const int qs = __builtin_amdgcn_readfirstlane(q);
                    const int r0 = qs * SY_U + 1;
                    const int need = r0 + SY_U - 1 + 63 + phi;
                    if (sf && q == q_lo + k9 && need > 256) {   // (until the producer nears my first block I am one more importer of this scout)
                        if (!s2_importer<OV>(sd, p, s, phi, UT, rows, gb, ngap, lane, false, S2Pace(), need - 192)) return;
                    }
                    while (lds_load(&sd.prod_u) < need)
                        if (spin.fail(p.abort_flag)) return;
                    asm volatile("" ::: "memory");
                    const u32 e0 = (u32)(r0 - 2 + lane + phi);        // ring entry of row r0 - 1
                    const bool flat = (((u32)(r0 - 2 + phi) & (SY_R - 1)) + 63 + SY_U) < (u32)SY_R;   // no lane wraps inside this block
                    const uint64_t bH = (uint64_t)(uintptr_t)(H + (((int64_t)r0 * M) << hsh)), bP = (uint64_t)(uintptr_t)(P + (int64_t)r0 * M * (p8 ? 1 : 4));
                    // (a short last block: the descriptors end with the matrix, the stores of the rows below it are dropped)
                    const int nbr = min(SY_U, rows - r0 + 1);
                    const int nrH = nbr == SY_U ? 0x7FFFFF00 : nbr * (int)rowbH, nrP = nbr == SY_U ? 0x7FFFFF00 : nbr * (int)rowbP;
                    const sw_i32x4 dH = {__builtin_amdgcn_readfirstlane((int)(u32)bH), __builtin_amdgcn_readfirstlane((int)(u32)(bH >> 32)), nrH, 0x00020000};
                    const sw_i32x4 dP = {__builtin_amdgcn_readfirstlane((int)(u32)bP), __builtin_amdgcn_readfirstlane((int)(u32)(bP >> 32)), nrP, 0x00020000};
                    u32 nz = (u32)(-(gb + ngap * (r0 - 1 + (int)jA)));
                    u32 bv = (u32)best, bi = 0;
                    const u32 eoff = (e0 & (SY_R - 1)) * 4u;
                    C2Out o;
                    if (wl) {   // the descriptors start at the 64-byte boundary below the block's first own cell
                        const int64_t c1 = (int64_t)s * W + 1;
                        const uint64_t fH = bH + (uint64_t)((c1 * 4) << hsh), fP = bP + (uint64_t)(c1 * 4);
                        const uint64_t bH2 = fH & ~(uint64_t)63, bP2 = fP & ~(uint64_t)63;
                        const u32 dlH = (u32)(bH2 - bH), dlP = (u32)(bP2 - bP);
                        const sw_i32x4 dH2 = {__builtin_amdgcn_readfirstlane((int)(u32)bH2), __builtin_amdgcn_readfirstlane((int)(u32)(bH2 >> 32)),
                                              nbr == SY_U ? 0x7FFFFF00 : __builtin_amdgcn_readfirstlane(nrH - (int)dlH), 0x00020000};
                        const sw_i32x4 dP2 = {__builtin_amdgcn_readfirstlane((int)(u32)bP2), __builtin_amdgcn_readfirstlane((int)(u32)(bP2 >> 32)),
                                              nbr == SY_U ? 0x7FFFFF00 : __builtin_amdgcn_readfirstlane(nrP - (int)dlP), 0x00020000};
                        // (int8 P: the legacy descriptor and byte offsets, from the lanes that own the strip's 110 columns only)
                        const u32 vH = voffH == SY_OOB ? SY_OOB : voffH - dlH;
                        const u32 vP = p8 ? ((voffP == SY_OOB || lane > (W >> 1)) ? SY_OOB : voffP) : (voffP == SY_OOB ? SY_OOB : voffP - dlP);
                        o.bm = consumer_block3(flat, nt, h64, p8, flat ? laneA + eoff : laneA, flat ? laneB + eoff : laneB, eoff, slot_addr, (u32)qs,
                                               __builtin_amdgcn_readfirstlane(qs == 0 ? 1 : 0), g0a, g0b, nz, (u32)aA, (u32)aB, mm_v, xm_v, ngap_v, vH, vP,
                                               dH2, p8 ? dP : dP2, rowbH, rowbP, bchars + (r0 - 1), wm, allod);
                        o.gla = o.glb = 0u;
                    } else
                    o = consumer_block2(flat, nt, p8, trk, h64, flat ? laneA + eoff : laneA, flat ? laneB + eoff : laneB, eoff, slot_addr, (u32)qs,
                                                    __builtin_amdgcn_readfirstlane(qs == 0 ? 1 : 0), g0a, g0b, nz, bv, bi, (u32)aA, (u32)aB, mm_v, xm_v, ngap_v,
                                                    voffH, voffP, dH, dP, rowbH, rowbP, bchars + (r0 - 1));
                    // (overlapping strips: the columns beyond the next strip's halo column are that strip's to report)
                    if (trk) { if (okB && mine && (int)bv > best) { best = (int)bv; bestq = qs; bestcode = (int)bi; } }
                    else if (okB && mine && (int)o.bm > best) { best = (int)o.bm; bestq = qs; }
                    if (p.bot_gran && qs == nblk - 1) {
                        // band-resident launch: the band's last row leaves as {tag, H} granules (the next band's halo row), then
                        // the flags of the two 63-column strips this strip covers (the interface counts 63-column strips)
                        const int zl = gb + ngap * (rows + (int)jA);
                        if (okA) __hip_atomic_store((gu64*)(p.bot_gran + jA), ((u64)p.bot_tag << 32) | (u64)(u32)((int)o.gla - zl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        if (okB) __hip_atomic_store((gu64*)(p.bot_gran + jB), ((u64)p.bot_tag << 32) | (u64)(u32)((int)o.glb - zl - ngap), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        if (s == 0 && lane == 0) __hip_atomic_store((gu64*)p.bot_gran, (u64)p.bot_tag << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        if (p.bot_done) {
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            const int n63 = (int)((p.cols + 62) / 63);
                            if (lane < 2 && 2 * s + lane < n63)
                                __hip_atomic_store((gu32*)(p.bot_done + 2 * s + lane), p.bot_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                    }
                }
                if (best > 0 && !nostore) {   // lowest row of block bestq holding the maximum, A before B: the lowest linear index
                    if (trk) {
                        bestrow = bestq * SY_U + 1 + (bestcode >> 1);
                        bestcol = bestcode & 1;
                    } else {
                        __builtin_amdgcn_s_waitcnt(0);
                        // Whole-line stores: only the cells this wave STORED count -- a cell of a line that is the neighbour's to write is the
                        // neighbour's to report (it computed the same value), and what memory holds there now may be anything.  inwin(): the
                        // test of C3_MASK for the piece `pc` bytes from the row's first own cell.
                        const u32 psz = h64 ? 16u : 8u, span = h64 ? 880u : 440u, lc = psz * (u32)(lane - 1);
                        const u32 f0 = (u32)(((uint64_t)(uintptr_t)H + (uint64_t)(((((int64_t)bestq * SY_U + 1) * M + (int64_t)s * W + 1) * 4) << hsh)) & 63u);
                        auto inwin = [&](u32 rowoff, u32 pc) { return (u32)(pc - ((f0 + rowoff + pc) & 63u)) < span; };
                        // (all 32 loads first, then the compares: one memory latency instead of sixteen at the end of every strip)
                        const int nk = min(SY_U, rows - bestq * SY_U);
                        int hvA[SY_U], hvB[SY_U];
#pragma unroll
                        for (int k = 0; k < SY_U; ++k) {
                            const int64_t o = (int64_t)(bestq * SY_U + 1 + min(k, nk - 1)) * M + jA;
                            hvA[k] = (int)__builtin_nontemporal_load(&H[o << hsh]);          // (int64: the low dword)
                            hvB[k] = (int)__builtin_nontemporal_load(&H[(o + 1) << hsh]);
                        }
#pragma unroll
                        for (int k = SY_U - 1; k >= 0; --k) {
                            bool stA = k < nk, stB = k < nk;
                            if (wl) {
                                const u32 rowoff = (u32)k * rowbH;
                                if (allod || (k & 1)) { stA = stA && inwin(rowoff, lc - psz / 2); stB = stB && lane < 63 && inwin(rowoff, lc + psz / 2); }   // (B rides in the next lane's shifted pair)
                                else stA = stB = stA && inwin(rowoff, lc);
                            }
                            if (stB && hvB[k] == best) { bestrow = bestq * SY_U + 1 + k; bestcol = 1; }
                            if (stA && hvA[k] == best) { bestrow = bestq * SY_U + 1 + k; bestcol = 0; }
                        }
                        if (bestrow == 0 && wlaunch) best = 0;   // (not among my stores: nothing to report)
                    }
                }
            } else
            for (int q = q_lo + k9; q < nblk; q += nc_eff) {
                const int r0 = q * SY_U + 1;
                const int need = r0 + SY_U - 1 + 63 + phi;       // lane 63's last row of the block
                while (lds_load(&sd.prod_u) < need)
                    if (spin.fail(p.abort_flag)) return;
                asm volatile("" ::: "memory");
                u32 gA[SY_U + 1], gB[SY_U + 1];
                const u32 e0 = (u32)(r0 - 2 + lane + phi);        // ring entry of row r0 - 1
                if ((((u32)(r0 - 2 + phi) & (SY_R - 1)) + 63 + SY_U) < (u32)SY_R) {   // no lane wraps inside this block
                    const u32* qa = rA + (e0 & (SY_R - 1));
                    const u32* qb = rB + (e0 & (SY_R - 1));
#pragma unroll
                    for (int k = 0; k <= SY_U; ++k) {
                        gA[k] = __hip_atomic_load(qa + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        gB[k] = __hip_atomic_load(qb + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k <= SY_U; ++k) {
                        gA[k] = __hip_atomic_load(rA + ((e0 + k) & (SY_R - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        gB[k] = __hip_atomic_load(rB + ((e0 + k) & (SY_R - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                asm volatile("" ::: "memory");
                lds_store(&lds.cons_blk[k9], q);                  // the ring entries are in registers: the producer may reuse them
                if (q == 0) {   // row 0 (H == 0) is known; lane 0 of the last strip (phi == 0) has no ring entry for it (local step 0)
                    gA[0] = (u32)(gb + ngap * (int)jA);
                    gB[0] = (u32)(gb + ngap * (int)jB);
                }
                const uint4 ch = *(const uint4*)(bchars + r0 - 1);     // wave-uniform: the block's 16 row characters (r0 - 1 is a multiple of 16)
                const u32 chw[4] = {ch.x, ch.y, ch.z, ch.w};
                const int nbr = min(SY_U, rows - r0 + 1), nrec = nbr == SY_U ? 0x7FFFFF00 : nbr * (int)rowb;
                const __amdgpu_buffer_rsrc_t rH = __builtin_amdgcn_make_buffer_rsrc((void*)(H + (int64_t)r0 * M), 0, nrec, 0x00020000);
                const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)((int32_t*)P + (int64_t)r0 * M), 0, nrec, 0x00020000);
                typedef int v2i __attribute__((ext_vector_type(2)));
                u32 zA = (u32)(gb + ngap * (r0 - 1 + (int)jA));
                int hAs[SY_U], hBs[SY_U];
#pragma unroll
                for (int k = 0; k < SY_U; ++k) {
                    const int c = (int)((chw[k >> 2] >> (8 * (k & 3))) & 0xffu);
                    zA += (u32)ngap;
                    const u32 zB = zA + (u32)ngap;
                    const u32 bl = (u32)__builtin_amdgcn_update_dpp(0, (int)gB[k], 0x138, 0xf, 0xf, false);   // lane l-1's B of the row above (wave_shr:1)
                    const u32 dA = bl + (u32)(aA == c ? mm : xm), dB = gA[k] + (u32)(aB == c ? mm : xm);
                    const int hA = (int)(gA[k + 1] - zA), hB = (int)(gB[k + 1] - zB);
                    int pA = (gA[k] == gA[k + 1]) ? 1 : 2, pB = (gB[k] == gB[k + 1]) ? 1 : 2;
                    pA = (dA == gA[k + 1]) ? 3 : pA;
                    pB = (dB == gB[k + 1]) ? 3 : pB;
                    pA = hA == 0 ? 0 : pA;
                    pB = hB == 0 ? 0 : pB;
                    v2i hv = {hA, hB}, pv = {pA, pB};
                    __builtin_amdgcn_raw_buffer_store_b64(hv, rH, (int)voff2, (int)(rowb * (u32)k), 0);
                    __builtin_amdgcn_raw_buffer_store_b64(pv, rP, (int)voff2, (int)(rowb * (u32)k), 0);
                    if (tail1) {
                        __builtin_amdgcn_raw_buffer_store_b32(hA, rH, (int)voff1, (int)(rowb * (u32)k), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(pA, rP, (int)voff1, (int)(rowb * (u32)k), 0);
                    }
                    hAs[k] = okA ? hA : 0;
                    hBs[k] = okB ? hB : 0;
                }
                // arg-max: block maximum first; the cell only when some lane improved (lowest row, then A before B: the lowest index)
                int bm = 0;
#pragma unroll
                for (int k = 0; k < SY_U; ++k) bm = max(bm, max(hAs[k], hBs[k]));
                if (__builtin_amdgcn_ballot_w64(bm > best) != 0) {
                    if (bm > best) {
                        best = bm;
#pragma unroll
                        for (int k = SY_U - 1; k >= 0; --k) {
                            if (hBs[k] == bm) { bestrow = r0 + k; bestcol = 1; }
                            if (hAs[k] == bm) { bestrow = r0 + k; bestcol = 0; }
                        }
                    }
                }
            }
            if (best > 0) atomicMax(p.result_key, ((u64)(u32)best << 40) | (SW_KEY_IDX_MASK - (u64)((int64_t)bestrow * M + jA + bestcol + p.idx_off)));
        } else if (importer) {
            // Behind scouts the fillers no longer wait for each other -- and the early ones, far ahead of any deadline, take their equal
            // share of the store bandwidth from the late ones, whose end is the end of the fill (16384^2: 131 fillers x 1008 bytes per row
            // at ~4.2 TB/s = 31 ns per row where the producer could do 26).  So a filler is paced to finish when the LAST one can at best:
            // (S - 1 - s) hand-offs later than it could by itself.  filler_hop_ps: the host's (low) estimate of a hand-off, 0 = no pacing.
            S2Pace pace;
            if (p.filler_hop_ps > 0 && nscout > 0 && !p.top_gran && !sf) {   // (a band that waits for its halo row starts when that arrives: no pacing; a scout is never paced)
                pace.on = true;
                pace.bps = s2_stride<OV>() * ((H ? (h64 ? 8 : 4) : 0) + (P ? (p8 ? 1 : 4) : 0));
                pace.steps = UT + 64;
                pace.S = S; pace.s = s;
                if (s == 0) pace.calibrate(p, 0.f);   // (strip 0 waits for nobody: the host's estimate)
            }
            if (!s2_importer<OV>(sd, p, s, phi, UT, rows, gb, ngap, lane, false, pace)) return;
        }
        __syncthreads();
    }
}

template <int NC, bool OV>
__global__ void __launch_bounds__(768) sw_systolic2(const unsigned char* seq_a, const unsigned char* seq_b, FillParams p) {
    __shared__ Sys2Lds lds;
    __shared__ S2Prep prep;
    const int nl = s2_prologue(prep, p, seq_a, seq_b);
    if (nl >= 0 && nl <= 7) {   // (more letters: sw_systolic, enqueued behind this launch, fills; < 0: the barrier gave up, the launch is aborted)
        const unsigned char* mine = p.priv + (int64_t)blockIdx.x * p.priv_stride;
        s2_body<NC, OV>(lds, prep.tab, mine, mine + p.bpad_pstride, seq_a, p);
    }
    s2_epilogue(p, nl <= 7);
}
template __global__ void sw_systolic2<4, false>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<4, true>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<5, false>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<5, true>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<6, false>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<6, true>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<7, false>(const unsigned char*, const unsigned char*, FillParams);
template __global__ void sw_systolic2<7, true>(const unsigned char*, const unsigned char*, FillParams);
