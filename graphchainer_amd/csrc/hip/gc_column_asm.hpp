// The column loop of one (node, slice) tile of the one-extension-per-wave whole-read kernel as ONE asm statement per (KIND, MODE)
// (computeTileW's lean path, gc_device_wave.hpp). Same arithmetic, same column order and same lane contents as the
// C++ lambda it replaced (commit 555b2d3 holds that one; computeTileW's generic loop, myersStep per column, is the readable statement
// of the recurrence); what changes is the per-column overhead around the recurrence:
//
// - match mask: the four masks sit in eight consecutive SGPRs and the column's 2-bit code, kept pre-shifted left by one, indexes them:
//   s_and_b32 m0, codes, 6 / s_lshr_b64 codes, 2 / s_movrels_b64 - three instructions where two s_bitcmp1 + three s_cselect_b64 + the
//   shift were six. The shift sits between the M0 write and s_movrels_b64 on purpose: gfx9 wants one wait state between an SALU
//   write of M0 and s_movrel* (LLVM's GCNHazardRecognizer::checkReadM0Hazards, one wait state where hasReadM0MovRelInterpHazard(),
//   which is every gfx9), nothing inside an asm string is padded, and an independent instruction in the gap is free.
// - the column number goes to M0 once per column (s_add_i32 m0, pos, k): M0 is the field descriptor of the s_bfe_u64 fetches of the
//   row above's carries (offset = bits 5:0, width = bit 16, carried in pos) and the lane select of the v_writelane that follow.
// - the loop is unrolled twice with a one-column tail: 1.5 instructions of loop control per column instead of 3.
// - the code stream changes word inside the statement. With the pre-shift a 64-bit stream holds 31 codes and a half, so a node has
//   three segments: columns 1..31 from w0 >> 1, columns 32..62 from w1 << 1, column 63 from w1 >> 61.
//
// An asm operand has no way to name one half of a 64-bit register pair, and the recurrence needs halves (the 64-bit add is
// s_add_u32 + s_addc_u32, the lane words are 32-bit), so everything that is addressed by halves lives in fixed registers:
// s[72:79] masks A C G T, s[80:81] VP, s[82:83] VN, s[84:85] / s[86:87] / s[88:89] temporaries, s[90:91] code stream.
// The rest (Eq, Xv, the carry word, counters) is left to the register allocator.
#pragma once

#define GC_CA_NL "\n\t"
// Eq = mask[code]; leaves the stream at the next column's code
#define GC_CA_SELECT \
	"s_and_b32 m0, s90, 6" GC_CA_NL "s_lshr_b64 s[90:91], s[90:91], 2" GC_CA_NL "s_movrels_b64 %[Eq], s[72:73]" GC_CA_NL
// One column. M0SET: M0 = pos + k. HN: carry-in of Mh from the row above, ORed into Eq (KIND 0, 1). HP: carry-in of Ph (constant 1 for KIND 2).
// HNMH: the same Mh carry into the shifted Mh (KIND 0, 1). FORCE: the forced first row (KIND 0). STORE: the column to the lanes (MODE 1, 2).
#define GC_CA_COLUMN(M0SET, HN, HP, HNMH, FORCE, STORE) \
	GC_CA_SELECT \
	M0SET GC_CA_NL \
	"s_or_b64 %[Xv], %[Eq], s[82:83]" GC_CA_NL \
	HN \
	"s_and_b64 s[84:85], %[Eq], s[80:81]" GC_CA_NL \
	"s_add_u32 s84, s84, s80" GC_CA_NL \
	"s_addc_u32 s85, s85, s81" GC_CA_NL \
	"s_xor_b64 s[84:85], s[84:85], s[80:81]" GC_CA_NL \
	"s_or_b64 s[84:85], s[84:85], %[Eq]" GC_CA_NL          /* Xh */ \
	"s_or_b64 %[Eq], s[84:85], s[80:81]" GC_CA_NL \
	"s_orn2_b64 s[86:87], s[82:83], %[Eq]" GC_CA_NL        /* Ph = VN | ~(Xh | VP) */ \
	"s_and_b64 s[88:89], s[80:81], s[84:85]" GC_CA_NL      /* Mh = VP & Xh */ \
	"v_writelane_b32 %[plus], s87, m0" GC_CA_NL \
	"v_writelane_b32 %[minus], s89, m0" GC_CA_NL \
	"s_lshl_b64 s[84:85], s[86:87], 1" GC_CA_NL \
	HP                                                     /* sPh */ \
	"s_lshl_b64 s[88:89], s[88:89], 1" GC_CA_NL \
	HNMH                                                   /* sMh */ \
	"s_or_b64 %[Eq], %[Xv], s[84:85]" GC_CA_NL \
	"s_orn2_b64 s[80:81], s[88:89], %[Eq]" GC_CA_NL        /* VP = sMh | ~(Xv | sPh) */ \
	"s_and_b64 s[82:83], s[84:85], %[Xv]" GC_CA_NL         /* VN = sPh & Xv */ \
	FORCE \
	STORE

#define GC_CA_HN "s_bfe_u64 %[hN], %[pHN], m0" GC_CA_NL "s_or_b64 %[Eq], %[Eq], %[hN]" GC_CA_NL
#define GC_CA_HP "s_bfe_u64 %[Eq], %[pHP], m0" GC_CA_NL "s_or_b64 s[84:85], s[84:85], %[Eq]" GC_CA_NL
#define GC_CA_HP_ONE "s_or_b32 s84, s84, 1" GC_CA_NL
#define GC_CA_HNMH "s_or_b64 s[88:89], s[88:89], %[hN]" GC_CA_NL
#define GC_CA_FORCE "s_bfe_u64 %[hN], %[forced], m0" GC_CA_NL "s_andn2_b64 s[80:81], s[80:81], %[hN]" GC_CA_NL "s_or_b64 s[82:83], s[82:83], %[hN]" GC_CA_NL
#define GC_CA_STORE \
	"v_writelane_b32 %[c0], s80, m0" GC_CA_NL "v_writelane_b32 %[c1], s81, m0" GC_CA_NL "v_writelane_b32 %[c2], s82, m0" GC_CA_NL "v_writelane_b32 %[c3], s83, m0" GC_CA_NL
#define GC_CA_NONE ""

// The loop. pos = column | 1 << 16 (the descriptor's width bit); endm1 = the segment's last column, nm1 = the node's last column, same form.
#define GC_CA_LOOP(HN, HP, HNMH, FORCE, STORE) \
	"s_lshr_b64 s[90:91], %[w0], 1" GC_CA_NL \
	"s_min_i32 %[endm1], %[nm1], 0x1001f" GC_CA_NL \
	"s_mov_b32 %[pos], 0x10001\n" \
	"1:" GC_CA_NL                                          /* a segment: pairs of columns while two are left */ \
	"s_cmp_ge_i32 %[pos], %[endm1]" GC_CA_NL \
	"s_cbranch_scc1 3f\n" \
	"2:" GC_CA_NL \
	GC_CA_COLUMN("s_mov_b32 m0, %[pos]", HN, HP, HNMH, FORCE, STORE) \
	GC_CA_COLUMN("s_add_i32 m0, %[pos], 1", HN, HP, HNMH, FORCE, STORE) \
	"s_add_i32 %[pos], %[pos], 2" GC_CA_NL \
	"s_cmp_lt_i32 %[pos], %[endm1]" GC_CA_NL \
	"s_cbranch_scc1 2b\n" \
	"3:" GC_CA_NL                                          /* the odd column */ \
	"s_cmp_gt_i32 %[pos], %[endm1]" GC_CA_NL \
	"s_cbranch_scc1 4f" GC_CA_NL \
	GC_CA_COLUMN("s_mov_b32 m0, %[pos]", HN, HP, HNMH, FORCE, STORE) \
	"s_add_i32 %[pos], %[pos], 1\n" \
	"4:" GC_CA_NL                                          /* next segment of the code stream, if the node goes on */ \
	"s_cmp_ge_i32 %[endm1], %[nm1]" GC_CA_NL \
	"s_cbranch_scc1 6f" GC_CA_NL \
	"s_bitcmp1_b32 %[endm1], 5" GC_CA_NL \
	"s_cbranch_scc1 5f" GC_CA_NL \
	"s_lshl_b64 s[90:91], %[w1], 1" GC_CA_NL \
	"s_min_i32 %[endm1], %[nm1], 0x1003e" GC_CA_NL \
	"s_branch 1b\n" \
	"5:" GC_CA_NL \
	"s_lshr_b64 s[90:91], %[w1], 61" GC_CA_NL \
	"s_mov_b32 %[endm1], %[nm1]" GC_CA_NL \
	"s_branch 1b\n" \
	"6:"

#define GC_CA_OUT_COMMON [VP] "+{s[80:81]}"(VP), [VN] "+{s[82:83]}"(VN), [plus] "+v"(plusWord), [minus] "+v"(minusWord), [Eq] "=&s"(Eq), [Xv] "=&s"(Xv), [pos] "=&s"(pos), [endm1] "=&s"(endm1)
#define GC_CA_OUT_STORE , [c0] "+v"(cr[0]), [c1] "+v"(cr[1]), [c2] "+v"(cr[2]), [c3] "+v"(cr[3])
#define GC_CA_IN_COMMON "{s[72:73]}"(eA), "{s[74:75]}"(eC), "{s[76:77]}"(eG), "{s[78:79]}"(eT), [w0] "s"(w0), [w1] "s"(w1), [nm1] "s"(nm1)
#define GC_CA_CLOBBER "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "m0", "scc"

#if defined(__HIP_DEVICE_COMPILE__)
// KIND / MODE as in computeTileW. Every argument is wave-uniform except the lane words (plusWord, minusWord, cr[0..3]).
template <int KIND, int MODE>
__device__ __forceinline__ void gcColumnLoopAsm(uint64_t eA, uint64_t eC, uint64_t eG, uint64_t eT, uint64_t& VP, uint64_t& VN, uint64_t prevHP, uint64_t prevHN, uint64_t forced,
	uint64_t w0, uint64_t w1, int nodeLength, uint32_t& plusWord, uint32_t& minusWord, uint32_t* cr)
{
	const uint32_t nm1 = (uint32_t)__builtin_amdgcn_readfirstlane((nodeLength - 1) | (1 << 16));
	uint64_t Eq, Xv, hN;
	uint32_t pos, endm1;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
	// (M0 is reserved to the compiler, which warns about the clobber; it is written and read inside the statement only)
	if constexpr (KIND == 2 && MODE == 0)
		asm(GC_CA_LOOP(GC_CA_NONE, GC_CA_HP_ONE, GC_CA_NONE, GC_CA_NONE, GC_CA_NONE)
			: GC_CA_OUT_COMMON : GC_CA_IN_COMMON : GC_CA_CLOBBER);
	else if constexpr (KIND == 2)
		asm(GC_CA_LOOP(GC_CA_NONE, GC_CA_HP_ONE, GC_CA_NONE, GC_CA_NONE, GC_CA_STORE)
			: GC_CA_OUT_COMMON GC_CA_OUT_STORE : GC_CA_IN_COMMON : GC_CA_CLOBBER);
	else if constexpr (KIND == 1 && MODE == 0)
		asm(GC_CA_LOOP(GC_CA_HN, GC_CA_HP, GC_CA_HNMH, GC_CA_NONE, GC_CA_NONE)
			: GC_CA_OUT_COMMON, [hN] "=&s"(hN) : GC_CA_IN_COMMON, [pHP] "s"(prevHP), [pHN] "s"(prevHN) : GC_CA_CLOBBER);
	else if constexpr (KIND == 1)
		asm(GC_CA_LOOP(GC_CA_HN, GC_CA_HP, GC_CA_HNMH, GC_CA_NONE, GC_CA_STORE)
			: GC_CA_OUT_COMMON, [hN] "=&s"(hN) GC_CA_OUT_STORE : GC_CA_IN_COMMON, [pHP] "s"(prevHP), [pHN] "s"(prevHN) : GC_CA_CLOBBER);
	else if constexpr (MODE == 0)
		asm(GC_CA_LOOP(GC_CA_HN, GC_CA_HP, GC_CA_HNMH, GC_CA_FORCE, GC_CA_NONE)
			: GC_CA_OUT_COMMON, [hN] "=&s"(hN) : GC_CA_IN_COMMON, [pHP] "s"(prevHP), [pHN] "s"(prevHN), [forced] "s"(forced) : GC_CA_CLOBBER);
	else
		asm(GC_CA_LOOP(GC_CA_HN, GC_CA_HP, GC_CA_HNMH, GC_CA_FORCE, GC_CA_STORE)
			: GC_CA_OUT_COMMON, [hN] "=&s"(hN) GC_CA_OUT_STORE : GC_CA_IN_COMMON, [pHP] "s"(prevHP), [pHN] "s"(prevHN), [forced] "s"(forced) : GC_CA_CLOBBER);
#pragma clang diagnostic pop
}
#endif
