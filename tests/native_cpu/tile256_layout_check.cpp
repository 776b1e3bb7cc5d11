// CPU check of fadtk_amd/csrc/tile256_layout.h: the partial-tile slot's element map against the accumulator layout of the
// 16x16x32 MFMA, the place of the diagonal, the sub-blocks a diagonal block issues, the stage image (LDS-DMA side against the
// transposed reads) and the banks of every transposed read.  Plain C++ (g++), no GPU.
#include "../../fadtk_amd/csrc/tile256_layout.h"
#include "../../fadtk_amd/csrc/tile256_roles.h"
#include <cstdio>
#include <set>
#include <vector>
using namespace fad::t256;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
    // 1. slot element -> (row, column): a bijection, and the C/D layout of v_mfma_f32_16x16x32: lane l, register r of sub-block
    //    (si, sj) -> row 16 si + 4 (l >> 4) + r, column 16 sj + (l & 15)
    {
        std::vector<int> seen(BLK, 0);
        for (int si = 0; si < 2; ++si)
            for (int sj = 0; sj < 2; ++sj)
                for (int l = 0; l < 64; ++l) {
                    const int e = slot_float4(si, sj, l);
                    CHECK(e >= 0 && e < 256, "float4 index %d", e);
                    for (int r = 0; r < 4; ++r) {
                        const int row = slot_row0(e) + r, col = slot_col(e);
                        CHECK(row == 16 * si + 4 * (l >> 4) + r && col == 16 * sj + (l & 15), "sub-block (%d, %d) lane %d reg %d -> (%d, %d)", si, sj, l, r, row, col);
                        if (row >= 0 && row < FR && col >= 0 && col < FR) ++seen[row * FR + col];
                    }
                }
        for (int i = 0; i < BLK; ++i) CHECK(seen[i] == 1, "element (%d, %d) named %d times", i / FR, i % FR, seen[i]);
        std::set<int> es;
        for (int si = 0; si < 2; ++si) for (int sj = 0; sj < 2; ++sj) for (int l = 0; l < 64; ++l) es.insert(slot_float4(si, sj, l));
        CHECK(es.size() == 256, "%zu distinct float4 of 256", es.size());
    }
    // 2. the diagonal pick-up names element (c, c)
    for (int c = 0; c < FR; ++c) {
        const int e = slot_float4(diag_sub(c), diag_sub(c), diag_lane(c));
        CHECK(slot_row0(e) + diag_comp(c) == c && slot_col(e) == c, "diagonal %d -> (%d, %d)", c, slot_row0(e) + diag_comp(c), slot_col(e));
        CHECK(diag_lane(c) >= 0 && diag_lane(c) < 64 && diag_comp(c) >= 0 && diag_comp(c) < 4, "diagonal %d: lane %d comp %d", c, diag_lane(c), diag_comp(c));
    }
    // 3. every element with row <= column of a diagonal block lies in an issued sub-block; off the diagonal all four are issued;
    //    MFMAs per stage and role: 33 / 33 / 35 / 35 / 32
    for (int row = 0; row < FR; ++row)
        for (int col = row; col < FR; ++col) CHECK(sub_block_issued(true, row >> 4, col >> 4), "(%d, %d) of a diagonal block not issued", row, col);
    CHECK(!sub_block_issued(true, 1, 0), "sub-block (1, 0) of a diagonal block is issued");
    for (int q = 0; q < 4; ++q) CHECK(sub_block_issued(false, q >> 1, q & 1), "sub-block %d of an off-diagonal block not issued", q);
    {
        auto count = [](const int* fa, const int* fb, int nb) {
            int n = 0;
            for (int b = 0; b < nb; ++b) for (int q = 0; q < 4; ++q) n += sub_block_issued(fa[b] == fb[b], q >> 1, q & 1);
            return n;
        };
        const int got[5] = {count(RoleDef<TRI_LO>::fa, RoleDef<TRI_LO>::fb, 9), count(RoleDef<TRI_HI>::fa, RoleDef<TRI_HI>::fb, 9),
                            count(RoleDef<RECT_C>::fa, RoleDef<RECT_C>::fb, 9), count(RoleDef<RECT_D>::fa, RoleDef<RECT_D>::fb, 9),
                            count(RoleDef<XR>::fa, RoleDef<XR>::fb, 8)};
        const int want[5] = {33, 33, 35, 35, 32};
        for (int i = 0; i < 5; ++i) CHECK(got[i] == want[i], "role %d issues %d MFMAs per stage, want %d", i, got[i], want[i]);
        std::printf("MFMAs per stage: %d %d %d %d %d\n", got[0], got[1], got[2], got[3], got[4]);
    }
    // 4. stage image: what the LDS-DMA writes (lane-linear rows) is where stage_byte looks for it -- a bijection per row that keeps
    //    every chunk in its slab and its 128-column window
    for (int wave = 0; wave < 8; ++wave)
        for (int p = 0; p < 4; ++p) {
            const int row = 4 * wave + p;
            std::set<int> chunks;
            for (int l = 0; l < 64; ++l) {
                const int c = dma_chunk(wave, p, l);
                chunks.insert(c);
                CHECK(stage_byte(row, 8 * c) == row * ROW_BYTES + 16 * l, "row %d: chunk %d written at lane %d, read at byte %d", row, c, l, stage_byte(row, 8 * c) - row * ROW_BYTES);
                CHECK((c >> 4) == (l >> 4), "row %d: chunk %d leaves its 128-column window", row, c);
            }
            CHECK(chunks.size() == 64, "row %d: %zu chunks", row, chunks.size());
        }
    // 5. transposed reads: lane 4 q + p of a 16-lane group names row q, columns 4 p .. 4 p + 3 of a 4 x 16 block; the block of group
    //    g and read j is rows 8 g + 4 j .. + 3 of the sub-fragment's 16 columns; the second read is the first + 4 rows; sub-fragment
    //    1 is sub-fragment 0 ^ 32 bytes; the two groups of each 32-lane half touch 64 distinct banks (bank = (byte / 4) % 64, 8 bytes
    //    = 2 banks per lane) -- for both reads and every fragment position of the 512-column row
    int reads = 0;
    for (int col0 = 0; col0 < 512; col0 += 16)
        for (int j = 0; j < 2; ++j) {
            for (int l = 0; l < 64; ++l) {
                const int g = l >> 4, q = (l & 15) >> 2, p = l & 3;
                const int a = tr_read_byte(l, j, col0);
                CHECK(a == stage_byte(8 * g + 4 * j + q, col0 + 4 * p), "col0 %d read %d lane %d: address %d", col0, j, l, a);
                CHECK(a % 8 == 0 && a >= 0 && a + 8 <= STAGE_ROWS * ROW_BYTES, "col0 %d read %d lane %d: address %d out of the stage or unaligned", col0, j, l, a);
                CHECK(lane_row0(l) == 8 * g, "lane %d holds rows from %d", l, lane_row0(l));
                if (j == 1) CHECK(a == tr_read_byte(l, 0, col0) + 4 * ROW_BYTES, "col0 %d lane %d: second read is not + 4 rows", col0, l);
                if (col0 & 16) CHECK(a == (tr_read_byte(l, j, col0 - 16) ^ 32), "col0 %d lane %d: sub-fragment 1 is not sub-fragment 0 ^ 32", col0, l);
                // the four elements behind the address are four adjacent columns of one row
                for (int k = 1; k < 4; ++k) CHECK(stage_byte(8 * g + 4 * j + q, col0 + 4 * p + k) == a + 2 * k, "col0 %d lane %d: columns not adjacent", col0, l);
            }
            for (int half = 0; half < 2; ++half) {
                std::set<int> banks;
                for (int l = 32 * half; l < 32 * half + 32; ++l) {
                    const int a = tr_read_byte(l, j, col0);
                    banks.insert((a / 4) % 64); banks.insert((a / 4 + 1) % 64);
                }
                CHECK(banks.size() == 64, "col0 %d read %d half %d: %zu banks of 64", col0, j, half, banks.size());
            }
            ++reads;
        }
    std::printf("%d transposed reads on 64 banks per half\n", reads);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("tile256 layout ok\n");
    return 0;
}
