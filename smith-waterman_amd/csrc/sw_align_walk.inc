// sw_align_walk.inc -- the walk of the canonical alignment (include/swhip.h) through its three states over the direction bytes in a
// wave's slot, and the store of the item's sw_alignment (gfx950): the statements that sw_align_affine_wave<C>, sw_align_hits_wave<C> and
// ak_align_hit<C> (sw_align_ckpt.hip) run once the arg-max of an item is known.  Each of them includes this file once; there is no
// other copy of the text.  (Text, not a function, for the reason sw_gotoh_sweep.inc gives; included, the kernels' instructions are those
// of the copies this file replaces -- DESIGN 9f.)  sw_align_dirfill.inc defines the direction byte and its open bits.
//
// The slot holds the rows bf .. bl of the item's direction matrix, row stride qpad, row bf at offset 0: the whole matrix (1 .. len) in
// the whole-matrix kernels, one band in the checkpointed ones.  Only the wave that wrote the slot reads it.  The includer has drained
// vmcnt -- its own stores have then reached the L2 -- and the matrix is read with sc1 loads only, which are served from the L2: the L1
// of the CU may still hold lines of the item that used the slot before.  The wave stages windows of SW_WIN rows x SW_WIN bytes in LDS
// (16 bytes per lane and load, coalesced; clipped to bf .. bl) that end at the cell it stands on, and takes a whole run per LDS round
// trip: in state H lane l looks at (i - l, j - l) and the ballot of "came from the diagonal" gives the length of the run of M; in state
// E / F lane l looks at the open bit l cells up / left and the first opener ends the run of D / I.  A look-back into a row above bf is
// "not known", like one beyond the window: the run ends there and the next round goes on from it.  It walks twice: once to count the
// ops and find the begin corner, once to write the ops in alignment order, left-justified (skipped where they do not all fit).  Nothing
// is written outside the item's ops_cap bytes.
//
// In scope where it is included, all wave-uniform but `lane` and voffL0:
//   int lane;  int len, qlen;  u32 qpad;  u64 score, pos;  int i1, j1  the item's arg-max (sw_align_dirfill.inc leaves them so);
//   __amdgpu_buffer_rsrc_t rD  the slot;  rO  the item's own ops_cap bytes (empty without ops);
//   int64_t ops_cap;  bool has_ops;  u32 voffL0 = lane == 0 ? 0 : SW_OOB;
//   sw_v4i* win  the wave's SW_WIN x SW_WIN bytes of LDS;  const unsigned char* winb  the same bytes;
//   walk_round_t  the type of the round counter: int or u64, each kernel family its own (the other one moves its instructions);
//   SW_WALK_BAND  a macro, #defined before the include and #undef'ed behind it.  It expands in every round before the window load,
//                 where  int ai, aj  (the cell the lanes look back from) and  int wr0, wcb  (the window) are in scope, and declares
//                 const int bf, bl.  Whole matrix: `const int bf = 1, bl = len;` and nothing else.  Checkpointed: if (ai, aj) has
//                 left the band in the slot, fill its band, drain vmcnt and forget the window (wr0 = wcb = 1 << 30); then bf, bl
//                 of the band now in the slot.
//   SW_WALK_ALN   a macro like it: an expression for the descriptor of the item's sw_alignment, expanded once, behind the walk.  (A
//                 macro and not a name rA in scope: the whole-matrix kernels build the descriptor there and the checkpointed ones
//                 ahead of the item; built at the other place, either family's scalar registers are allotted differently.)
// It leaves int i0, j0 (the begin corner) and nops, and has stored the item's sw_alignment and, where they fit, its ops.
        int i0 = 0, j0 = 0, nops = 0;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1 && (nops == 0 || !has_ops || (int64_t)nops > ops_cap)) break;
            int i = i1, j = j1, state = 0, n = 0;
            int wr0 = 1 << 30, wcb = 1 << 30;      // first row and first byte column of the window in LDS (none yet)
            bool done = score == 0;
            // `cnt` ops `ch` behind the n already taken: the walk goes backwards, op k from the end lies at nops - 1 - k
            auto emit = [&](int cnt, int ch) {
                if (pass == 1) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)ch, rO, lane < cnt ? nops - 1 - n - lane : (int)SW_OOB, 0, 0);
                n += cnt;
            };
            // (every round takes at least one op or changes the state once per op: the bound is never reached, it only keeps damaged
            //  direction bytes from holding the wave)
            const walk_round_t rounds = 2 * ((walk_round_t)len + (walk_round_t)qlen) + 8;
            for (walk_round_t round = 0; !done && round < rounds; ++round) {
                if (i < 1 || j < 1) break;          // H at the edge of the matrix: 0 (E and F leave for H before they get here)
                // the cell the lanes look back from: (i, j) in H, one up in E, one left in F
                const int ai = state == 2 ? i - 1 : i, aj = state == 3 ? j - 1 : j;
                SW_WALK_BAND
                if (ai >= 1 && aj >= 1 && (ai < wr0 || aj - 1 < wcb)) {
                    wr0 = ai - (SW_WIN - 1);
                    wcb = ((aj - 1) & ~15) - (SW_WIN - 16);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    sw_v4i v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = wr0 + 16 * q + (lane >> 2), cb = wcb + 16 * (lane & 3);
                        const bool in = row >= bf && row <= bl && cb >= 0;
                        v[q] = __builtin_amdgcn_raw_buffer_load_b128(rD, in ? (int)((u32)(row - bf) * qpad + (u32)cb) : (int)SW_OOB, 0, SW_SC1);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) win[(16 * q + (lane >> 2)) * (SW_WIN / 16) + (lane & 3)] = v[q];
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                // lane l: the cell l steps back along the state's direction; `known`: outside the matrix (a fixed answer) or in the window
                // AND in the slot -- a row above bf is not known until its band has been filled
                const int r = state == 3 ? ai : ai - lane, c = state == 2 ? aj : aj - lane;
                const bool inside = r >= 1 && c >= 1, inwin = inside && r >= wr0 && r >= bf && c - 1 >= wcb;
                const bool known = !inside || inwin;
                const int b = inwin ? (int)winb[(r - wr0) * SW_WIN + (c - 1 - wcb)] : 0;
                if (state == 0) {
                    const u64 notdiag = ~__builtin_amdgcn_ballot_w64(known && (b & 3) == 1);
                    const int run = notdiag ? (int)__builtin_ctzll(notdiag) : 64;
                    emit(run, 'M');
                    i -= run; j -= run;
                    if (run < 64 && __builtin_amdgcn_readlane((int)known, run)) {
                        const int src = __builtin_amdgcn_readlane(b, run) & 3;
                        if (src == 0) done = true; else state = src;
                    }
                } else {
                    const bool open = !inside || (b & (state == 2 ? 4 : 8)) != 0;
                    const u64 stop = __builtin_amdgcn_ballot_w64(!known || open);
                    const int first = stop ? (int)__builtin_ctzll(stop) : 64;
                    // lanes 0 .. first - 1 extend; lane `first` opens (one more op, back to H) or lies beyond what is known
                    const bool opens = first < 64 && __builtin_amdgcn_readlane((int)known, first);
                    const int cnt = first + (opens ? 1 : 0);
                    emit(cnt, state == 2 ? 'D' : 'I');
                    if (state == 2) i -= cnt; else j -= cnt;
                    if (opens) state = 0;
                }
            }
            if (pass == 0) { nops = n; i0 = i; j0 = j; }
        }
        {
            const __amdgpu_buffer_rsrc_t rA = SW_WALK_ALN;
            const bool any = score != 0;
            const sw_v4i v0 = {(int)(u32)pos, (int)(u32)(pos >> 32), (int)(u32)score, 0};
            const sw_v4i v1 = {any ? j0 : 0, 0, any ? i0 : 0, 0};
            const sw_v4i v2 = {any ? j1 : 0, 0, any ? i1 : 0, 0};
            __builtin_amdgcn_raw_buffer_store_b128(v0, rA, (int)voffL0, 0, 0);                    // max_pos, max_score
            __builtin_amdgcn_raw_buffer_store_b128(v1, rA, (int)voffL0, 16, 0);                   // q_begin, t_begin
            __builtin_amdgcn_raw_buffer_store_b128(v2, rA, (int)voffL0, 32, 0);                   // q_end, t_end
            __builtin_amdgcn_raw_buffer_store_b64(sw_v2i{nops, 0}, rA, (int)voffL0, 48, 0);       // nops
        }
