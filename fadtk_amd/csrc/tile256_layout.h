// Where things sit in the 256-column-slab E^T E kernel (moments_tile256.h) -- plain constexpr C++, shared by the kernel (LDS-DMA
// side, transposed reads, epilogue, the guard's pick-up of the diagonal), by moments_reduce256 and by the CPU check
// (tests/native_cpu/tile256_layout_check.cpp).  Who owns which 32 x 32 block is in tile256_roles.h.
//
// Stage image.  A stage is 32 rows of 1 KiB: 64 chunks of 16 bytes = 8 float16 columns each (chunks 0..31 slab A, 32..63 slab B).
// A 32-column fragment is multiplied as two SUB-FRAGMENTS of 16 columns x 32 rows, the operand of v_mfma_f32_16x16x32_{f16,bf16}:
// lane l holds column 16 s + (l & 15) and the eight rows 8 (l >> 4) .. + 7 of the stage.  One ds_read_b64_tr_b16 gives a 16-lane
// group 4 rows x 16 columns, so a sub-fragment takes two of them (rows + 0..3, rows + 4..7), and the two groups of a 32-lane half
// read the SAME 32 bytes of rows that are 8 apart.  ds_read_b64_tr_b16 banks per 32-lane half, bank = (byte / 4) % 64, and a row
// is 1 KiB = 0 (mod 64 banks): the eight rows of a half -- row & 3 = 0..3, (row >> 3) & 1 = 0, 1 -- have to land in the eight
// different 32-byte places of a 256-byte window.  Hence the swizzle
//
//     chunk' = chunk ^ 2 (row & 3) ^ 8 ((row >> 3) & 1)
//
// (bits 1..3 of the chunk index: inside a 128-column window, a slab never mixes with the other).  Rows r and r + 4 swizzle alike,
// so the second read of a sub-fragment is the first + 4 KiB.  On the LDS-DMA side piece p of wave w is row 4 w + p: the term in
// row & 3 is the piece, the term in (row >> 3) & 1 = (w >> 1) & 1 is wave-uniform; both fold into the lane's source offsets.
//
// Partial-tile slot.  A block's 1 024 floats are 256 float4: float4 e = 64 (2 si + sj) + l is lane l's accumulator of the 16 x 16
// sub-block (si, sj) -- rows 16 si + 4 (l >> 4) + 0..3 of column 16 sj + (l & 15), the C/D layout of the 16x16x32 MFMA.  Sub-block
// (1, 0) of a DIAGONAL block (below the diagonal) is never issued: it stays zero, and the reduce takes row <= column only.
#pragma once
#include <cstdint>

namespace fad {
namespace t256 {

constexpr int STAGE_ROWS = 32;     // rows per stage
constexpr int ROW_BYTES = 1024;    // bytes per LDS row of a stage

// ---- stage image
constexpr int swizzle_of_row(int row) { return ((row & 3) << 1) | (((row >> 3) & 1) << 3); }
constexpr int swizzled_chunk(int row, int chunk) { return chunk ^ swizzle_of_row(row); }
// byte offset inside a stage of column `col` (0..511: slab A, then slab B) of row `row`
constexpr int stage_byte(int row, int col) { return row * ROW_BYTES + (swizzled_chunk(row, col >> 3) << 4) + (col & 7) * 2; }
// the chunk of its row that lane `lane` of LDS-DMA piece `piece` of wave `wave` FETCHES (the DMA writes lane-linear)
constexpr int dma_chunk(int wave, int piece, int lane) { return lane ^ swizzle_of_row(4 * wave + piece); }
// first of the eight stage rows lane `lane` holds of every sub-fragment
constexpr int lane_row0(int lane) { return 8 * (lane >> 4); }
// address lane `lane` supplies to transposed read `j` (0, 1) of the sub-fragment whose first column in the LDS row is `col0`
// (a multiple of 16): lane 4 q + p of a 16-lane group names row q, columns 4 p .. 4 p + 3 of the group's 4 x 16 block
constexpr int tr_read_byte(int lane, int j, int col0) {
    return stage_byte(lane_row0(lane) + 4 * j + ((lane & 15) >> 2), col0 + 4 * (lane & 3));
}

// ---- partial-tile slot: float4 index e (0..255), component r (0..3) -> row, column of the 32 x 32 block
constexpr int slot_float4(int si, int sj, int lane) { return 64 * (2 * si + sj) + lane; }
constexpr int slot_row0(int e) { return 16 * (e >> 7) + 4 * ((e & 63) >> 4); }      // component r: row slot_row0(e) + r
constexpr int slot_col(int e) { return 16 * ((e >> 6) & 1) + (e & 15); }
constexpr bool sub_block_issued(bool diagonal, int si, int sj) { return !(diagonal && si == 1 && sj == 0); }
// diagonal element (c, c): which lane holds it, in which sub-block (si = sj) and which component of its float4
constexpr int diag_sub(int c) { return c >> 4; }
constexpr int diag_lane(int c) { return 16 * ((c & 15) >> 2) + (c & 15); }
constexpr int diag_comp(int c) { return c & 3; }

}  // namespace t256
}  // namespace fad
