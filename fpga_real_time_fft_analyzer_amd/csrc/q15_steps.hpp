// q15_steps.hpp -- the instruction text of the integer cascades' pinned loops (cascade_q15.hip), preprocessor only: no
// types, no includes, so that the micro-benchmarks under tools/ubench time the text that ships.  Register arguments are
// complete operand texts ("v52", "%[y0]"); the named operands (%[s2], %[t], %[p0] .. %[p4], %[u], the taps, %[k]) are
// bound by the asm statement that expands the macros.
#pragma once

// ------------------------------------------------------------------------------------------ Q7 step (FPGA-exact)
// One block = one time step, written in the cyclic order the issue logic likes best.  With x = the LEFT neighbour's
// output (read in place by the DPP forms), y = the lane's own, and per step
//     y[n] = s2 + t,    t = t(B2, x[n]) - t(A1, y[n-1]),    s2 = t(B1, x[n-1]) + t(B0, x[n-2]) - t(A0, y[n-2])
// the block FIRST finishes y[n] from the t and s2 the previous block prepared (H), then starts everything of
// y[n+1] and y[n+2] that hangs on it:
//     H  y   = (int16)(s2 + t)                 G  u  = hi(p1) + hi(p2)        (terms of the block before)
//     B  p2  = x[n-1] * B0   (dpp)             C  p0 = x[n] * B2   (dpp; the neighbour's H is 3 instructions old)
//     A  p4  = y * -A1 + k                     I9 s2 = u + hi(p3)
//     D  p1  = x[n] * B1     (dpp)             F  t  = hi(p0) + hi(p4)
//     E  p3  = y * -A0 + k
// Y: the lane's output register of this step, H1: of the step before.
#define SA_Q7I_H(Y) "v_add_u32_sdwa " Y ", %[s2], %[t] dst_sel:WORD_0 dst_unused:UNUSED_SEXT src0_sel:DWORD src1_sel:DWORD\n\t"
#define SA_Q7I_G "v_add_u32_sdwa %[u], %[p1], %[p2] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1\n\t"
#define SA_Q7I_B(H1) "v_mul_i32_i24_dpp %[p2], " H1 ", %[cB0] row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
#define SA_Q7I_C(Y) "v_mul_i32_i24_dpp %[p0], " Y ", %[cB2] row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
#define SA_Q7I_A(Y) "v_mad_i32_i24 %[p4], " Y ", %[nA1], %[k]\n\t"
#define SA_Q7I_I9 "v_add_u32_sdwa %[s2], %[u], %[p3] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1\n\t"
#define SA_Q7I_D(Y) "v_mul_i32_i24_dpp %[p1], " Y ", %[cB1] row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
#define SA_Q7I_F "v_add_u32_sdwa %[t], %[p0], %[p4] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1\n\t"
#define SA_Q7I_E(Y) "v_mad_i32_i24 %[p3], " Y ", %[nA0], %[k]\n\t"
// I of the seven-instruction block: s2 = hi(p2) + hi(p3), no u
#define SA_Q7I_I "v_add_u32_sdwa %[s2], %[p2], %[p3] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1\n\t"

// Nine instructions, order H G B C A I D F E.  No instruction reads a register written by either of the two
// instructions in front of it except F -> H of the next block (one in between); the DPP read of the y just written has
// two instructions in between, which is what the hardware asks for (the compiler cannot see into an asm block and must
// not be relied on to pad).  tools/ubench/q7_step_rate.hip times these nine instructions alone, one wave per SIMD:
// 19.5 ns per step in this order, 24.1 ns in the order A B C D E F G H I (y finished second to last, its first reader
// one instruction later).
#define SA_Q7_BLOCK9(Y, H1) SA_Q7I_H(Y) SA_Q7I_G SA_Q7I_B(H1) SA_Q7I_C(Y) SA_Q7I_A(Y) SA_Q7I_I9 SA_Q7I_D(Y) SA_Q7I_F SA_Q7I_E(Y)

// The same block when the port tap B1 is zero in BOTH coefficient sets (the fixed ALPHA / BETA cascade of mode 0x00,
// imp/filter_pkg.vhd:54-68; the identity stages have B1 = 0 anyway): t(0, v) = 0 exactly, so the product D and the add G
// drop out and s2 = hi(p2) + hi(p3) is one instruction, issued BEFORE this block's B and E overwrite the previous
// block's p2 and p3.  Seven instructions per step, bit-identical results (new/filter_iir_cust.vhd:96-117 truncates every
// product separately: a zero tap contributes a zero term); %[p1], %[u] and %[cB1] are not mentioned.
// Order H I B A C E F (six orders and every single s_nop position were timed on the real kernel: this one, unpadded, is
// the fastest; profiles/r3_fuzz_and_soak.txt).
#define SA_Q7_BLOCK7(Y, H1) SA_Q7I_H(Y) SA_Q7I_I SA_Q7I_B(H1) SA_Q7I_A(Y) SA_Q7I_C(Y) SA_Q7I_E(Y) SA_Q7I_F

// eight steps: the lane's last eight outputs live in v52..v59 (named registers: the two 16-byte stores of lane 8 need
// them consecutive, and an asm operand cannot be addressed by sub-register)
#define SA_Q7_STEPS8(BLK)                                                                                              \
    BLK("v52", "v59") BLK("v53", "v52") BLK("v54", "v53") BLK("v55", "v54")                                            \
    BLK("v56", "v55") BLK("v57", "v56") BLK("v58", "v57") BLK("v59", "v58")

// Per group: select the refill into t, request the next refill (16-bit LDS read, used one group later: lgkmcnt(2) =
// everything but the two stores behind it), eight blocks, lane 8's eight outputs stored under an exec mask (restored
// five instructions before the next DPP read, as the hardware asks).  They are stored as sign-extended dwords; the
// saturating pack to int16 happens once per sample in the flush, where all 64 lanes have work, instead of four times
// per group here, where lane 8 of each row is the only one with a use for it.
#define SA_Q7_GROUP(BLK, RD_OFF, WR_OFF0, WR_OFF1)                                                                     \
    "s_waitcnt lgkmcnt(2)\n\t"                                                                                         \
    "v_cndmask_b32_e64 %[t], %[t], %[xin], %[inm]\n\t"                                                                 \
    "ds_read_u16 %[xin], %[xa] offset:" RD_OFF "\n\t"                                                                  \
    SA_Q7_STEPS8(BLK)                                                                                                  \
    "s_and_saveexec_b64 %[sv], %[outm]\n\t"                                                                            \
    "ds_write_b128 %[ra], v[52:55] offset:" WR_OFF0 "\n\t"                                                             \
    "ds_write_b128 %[ra], v[56:59] offset:" WR_OFF1 "\n\t"                                                             \
    "s_mov_b64 exec, %[sv]\n\t"

// the end of a tile loop's pass, both cascades: four groups on, next pass or out with nothing in flight
#define SA_TILE_LOOP_TAIL(RA_STEP)                                                                                     \
    "v_add_u32 %[xa], 64, %[xa]\n\t"                                                                                   \
    "v_add_u32 %[ra], " RA_STEP ", %[ra]\n\t"                                                                          \
    "s_add_i32 %[cnt], %[cnt], -1\n\t"                                                                                 \
    "s_cmp_lg_u32 %[cnt], 0\n\t"                                                                                       \
    "s_cbranch_scc1 1b\n\t"                                                                                            \
    "s_waitcnt lgkmcnt(0)\n\t"

// %[cnt] x 4 groups of a tile as ONE asm statement.  A lone wave issues at most one instruction per turn of its SIMD
// and stalls whole turns; which turns are lost depends on where the 8-byte instructions lie relative to the
// instruction fetch (tools/ubench/q7_nop_sweep.py: the same nine instructions run 19.4, 21.7 or 24.1 ns per step
// depending on a 4-byte s_nop in front of them or between them), so the loop is pinned: 64-byte aligned, nothing of
// the compiler's inside it (fourteen placements of a 4-byte `s_nop 0` inside the block were timed on the real kernel,
// 424-460 us: none beats the unpadded block in the order H G B C A I D F E).
#define SA_Q7_TILE(BLK)                                                                                                \
    "v_mov_b32 v52, %[y0]\n\tv_mov_b32 v53, %[y1]\n\tv_mov_b32 v54, %[y2]\n\tv_mov_b32 v55, %[y3]\n\t"                 \
    "v_mov_b32 v56, %[y4]\n\tv_mov_b32 v57, %[y5]\n\tv_mov_b32 v58, %[y6]\n\tv_mov_b32 v59, %[y7]\n\t"                 \
    "ds_read_u16 %[xin], %[xa]\n\t"                                                                                    \
    "s_waitcnt lgkmcnt(0)\n\t" /* first group: nothing in flight, lgkmcnt(2) passes */                                 \
    ".p2align 6\n"                                                                                                     \
    "1:\n\t"                                                                                                           \
    SA_Q7_GROUP(BLK, "16", "0", "16") SA_Q7_GROUP(BLK, "32", "32", "48") SA_Q7_GROUP(BLK, "48", "64", "80")            \
    SA_Q7_GROUP(BLK, "64", "96", "112")                                                                                \
    SA_TILE_LOOP_TAIL("0x80")                                                                                          \
    "v_mov_b32 %[y0], v52\n\tv_mov_b32 %[y1], v53\n\tv_mov_b32 %[y2], v54\n\tv_mov_b32 %[y3], v55\n\t"                 \
    "v_mov_b32 %[y4], v56\n\tv_mov_b32 %[y5], v57\n\tv_mov_b32 %[y6], v58\n\tv_mov_b32 %[y7], v59"

// ------------------------------------------------------------------------------------------ wide Q2.14 step
// block e of a group: PP = the pair of block e - 1, PC = this block's, (XC, XP) = the neighbour pair registers of this /
// the previous block, (WC, WP) = the unsaturated outputs likewise.  SEL: the refill select of the group's first block.
#define SA_W14_BLOCK(PP, PC, XC, XP, WC, WP, SEL)                                                                      \
    "v_dot2_i32_i16 %[al], " PP ", %[cfbl], %[k]\n\t"                                                                  \
    "v_dot2_i32_i16 %[ah], " PP ", %[cfbh], 0\n\t"                                                                     \
    "v_mov_b32_dpp " XC ", " PP " row_ror:1 row_mask:0xf bank_mask:0xf\n\t"                                            \
    "v_dot2_i32_i16 %[al], " XC ", %[c01l], %[al]\n\t"                                                                 \
    "v_dot2_i32_i16 %[ah], " XC ", %[c01h], %[ah]\n\t"                                                                 \
    "v_dot2_i32_i16 %[al], " XP ", %[c2l], %[al]\n\t"                                                                  \
    "v_dot2_i32_i16 %[ah], " XP ", %[c2h], %[ah]\n\t"                                                                  \
    "v_ashrrev_i32 %[al], 14, %[al]\n\t"                                                                               \
    "v_add_u32 " WC ", %[ah], %[al]\n\t" SEL                                                                           \
    "v_cvt_pk_i16_i32 " PC ", " WP ", " WC "\n\t"
// pair registers: odd blocks v52..v55 (what lane 8 stores), even blocks v56..v59
#define SA_W14_GROUP(RD_OFF, WR_OFF)                                                                                   \
    "s_waitcnt lgkmcnt(1)\n\t"                                                                                         \
    SA_W14_BLOCK("v55", "v56", "%[x0]", "%[x1]", "%[w0]", "%[w1]", "v_cndmask_b32_e64 %[w0], %[w0], %[xin], %[inm]\n\t") \
    "ds_read_i16 %[xin], %[xa] offset:" RD_OFF "\n\t"                                                                  \
    SA_W14_BLOCK("v56", "v52", "%[x1]", "%[x0]", "%[w1]", "%[w0]", "")                                                 \
    SA_W14_BLOCK("v52", "v57", "%[x0]", "%[x1]", "%[w0]", "%[w1]", "")                                                 \
    SA_W14_BLOCK("v57", "v53", "%[x1]", "%[x0]", "%[w1]", "%[w0]", "")                                                 \
    SA_W14_BLOCK("v53", "v58", "%[x0]", "%[x1]", "%[w0]", "%[w1]", "")                                                 \
    SA_W14_BLOCK("v58", "v54", "%[x1]", "%[x0]", "%[w1]", "%[w0]", "")                                                 \
    SA_W14_BLOCK("v54", "v59", "%[x0]", "%[x1]", "%[w0]", "%[w1]", "")                                                 \
    SA_W14_BLOCK("v59", "v55", "%[x1]", "%[x0]", "%[w1]", "%[w0]", "")                                                 \
    "s_and_saveexec_b64 %[sv], %[outm]\n\t"                                                                            \
    "ds_write_b128 %[ra], v[52:55] offset:" WR_OFF "\n\t"                                                              \
    "s_mov_b64 exec, %[sv]\n\t"
// the refill is requested one group ahead (lgkmcnt(1): everything but the store behind it)
#define SA_W14_TILE                                                                                                    \
    "v_mov_b32 v56, %[p0]\n\tv_mov_b32 v52, %[p1]\n\tv_mov_b32 v57, %[p2]\n\tv_mov_b32 v53, %[p3]\n\t"                 \
    "v_mov_b32 v58, %[p4]\n\tv_mov_b32 v54, %[p5]\n\tv_mov_b32 v59, %[p6]\n\tv_mov_b32 v55, %[p7]\n\t"                 \
    "ds_read_i16 %[xin], %[xa]\n\t"                                                                                    \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                         \
    ".p2align 6\n"                                                                                                     \
    "1:\n\t"                                                                                                           \
    SA_W14_GROUP("16", "0") SA_W14_GROUP("32", "16") SA_W14_GROUP("48", "32") SA_W14_GROUP("64", "48")                 \
    SA_TILE_LOOP_TAIL("64")                                                                                            \
    "v_mov_b32 %[p0], v56\n\tv_mov_b32 %[p1], v52\n\tv_mov_b32 %[p2], v57\n\tv_mov_b32 %[p3], v53\n\t"                 \
    "v_mov_b32 %[p4], v58\n\tv_mov_b32 %[p5], v54\n\tv_mov_b32 %[p6], v59\n\tv_mov_b32 %[p7], v55"
