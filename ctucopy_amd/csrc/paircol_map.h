// The index maps of the pair-column second stage of phase 1 (frontend_kernel.h, the DUAL block): plain C++, no HIP.
//
// Stage 1 of the packed DUAL block leaves element (k1, pass, fg, n2) of a step in lane 16 fg + n2, register k1, half `pass`.  Stage 2 runs
// one frame's two MIRROR columns in the two halves of a lane's register pairs: lane (f8, p), f8 = 4 pass + fg the frame slot of the step,
// p = 0..7 the pair, low half = column c_lo(p), high half = column c_hi(p).  (c_lo, c_hi) = (p, 16 - p) for p = 1..7 and (0, 8) for p = 0,
// so the bin Z[256 - k] that the untangle pairs with Z[k] is always in the same lane: for p >= 1 in the other half, for p = 0 (the two
// columns that mirror onto themselves) in the same half.
//
// The transpose between the stages goes through the wave's eight P rows (2080 dwords).  Row k1 of pass `pass` starts at dword
// PASS_B * pass + ROW * row_of(k1) and is written linear in the stage-1 lane.  row_of puts c_hi(p) right behind c_lo(p), so one
// ds_read2_b32 (offset0 = n2, offset1 = D + n2) fills a register pair with the (low, high) values of an element.  A stage-2 lane reads
// from dword read_dword(lane): lanes of one half wave (lane bits [4:0] = pass, fg & 1, p) start at banks 2 p + 16 (fg & 1) + 17 pass
// (mod 32), all 32 of them distinct, and every offset shifts them together.
#pragma once

namespace paircol {

constexpr int ROW = 65;        // dwords from one row to the next: 64 (four frames x 16 n2) + 1
constexpr int D = ROW;         // dwords from column c_lo(p)'s row to column c_hi(p)'s
constexpr int PASS_B = 1041;   // dwords from a row of pass A to the same row of pass B: 16 rows + 1, = 17 (mod 32)
constexpr int AREA = 2080;     // dwords of a wave's eight P rows (8 x PSTRIDE)
constexpr int NBIN = 257;      // bins 0..256 of a frame's power spectrum

constexpr int c_lo(int p) { return p; }
constexpr int c_hi(int p) { return p == 0 ? 8 : 16 - p; }
constexpr int column(int p, int half) { return half ? c_hi(p) : c_lo(p); }
constexpr int row_of(int k1) { return k1 == 0 ? 0 : k1 == 8 ? 1 : k1 < 8 ? 2 * k1 : 2 * (16 - k1) + 1; }
constexpr int store_byte(int k1, int pass) { return 4 * (PASS_B * pass + ROW * row_of(k1)); }  // + 4 * (16 fg + n2)

// stage-2 lane <-> (frame slot f8 = 4 pass + fg, pair p): bit 5 = fg >> 1, bit 4 = pass, bit 3 = fg & 1, bits [2:0] = p
constexpr int lane_of(int f8, int p) { return (((f8 & 3) >> 1) << 5) | ((f8 >> 2) << 4) | ((f8 & 1) << 3) | p; }
constexpr int lane_p(int lane) { return lane & 7; }
constexpr int lane_f8(int lane) { return 4 * ((lane >> 4) & 1) + 2 * (lane >> 5) + ((lane >> 3) & 1); }
constexpr int read_dword(int lane) { return PASS_B * (lane_f8(lane) >> 2) + ROW * 2 * lane_p(lane) + 16 * (lane_f8(lane) & 3); }  // + n2 | + D + n2

// The untangle.  Register k2 = 0..7 of half `half` of lane p holds Z[k], k = bin(p, half, k2); its partner Z[256 - k] (Z[256] = Z[0]) is
// register mirror_reg of half mirror_half of the same lane.  The twiddle W512^k of the bin is entry k2 of the LC_UT part of the per-lane
// constant record of the bin's column (layout_constants.h): record twiddle_record(p, half).
constexpr int bin(int p, int half, int k2) { return column(p, half) + 16 * k2; }
constexpr int mirror_half(int p, int half) { return p == 0 ? half : 1 - half; }
constexpr int mirror_reg(int p, int half, int k2) { return (p == 0 && half == 0) ? (16 - k2) & 15 : 15 - k2; }
constexpr int twiddle_record(int p, int half) { return column(p, half); }

constexpr bool rows_fit() {
    bool seen[16] = {};
    for (int k1 = 0; k1 < 16; k1++) {
        const int r = row_of(k1);
        if (r < 0 || r > 15 || seen[r]) return false;
        seen[r] = true;
        for (int pass = 0; pass < 2; pass++) {
            const int first = store_byte(k1, pass) / 4;
            if (first < 0 || first + 64 > AREA || store_byte(k1, pass) + 4 * 63 >= 65536) return false;
            if (pass == 1 && first < ROW * 15 + 64) return false;  // pass B starts behind pass A's last row
        }
    }
    return true;
}
constexpr bool reads_match_stores() {  // what lane (f8, p) reads at offsets n2 and D + n2 is element (column, pass, fg, n2) as stage 1 stored it
    for (int lane = 0; lane < 64; lane++) {
        const int f8 = lane_f8(lane), p = lane_p(lane);
        if (lane_of(f8, p) != lane) return false;
        for (int half = 0; half < 2; half++)
            for (int n2 = 0; n2 < 16; n2++)
                if (read_dword(lane) + half * D + n2 != store_byte(column(p, half), f8 >> 2) / 4 + 16 * (f8 & 3) + n2) return false;
    }
    return D + 15 <= 255;
}
constexpr bool mirrors_match() {
    for (int p = 0; p < 8; p++)
        for (int half = 0; half < 2; half++)
            for (int k2 = 0; k2 < 8; k2++)
                if (column(p, mirror_half(p, half)) + 16 * mirror_reg(p, half, k2) != (256 - bin(p, half, k2)) % 256) return false;
    return true;
}
constexpr bool bins_once() {  // each (lane, half, k2) stores bins k and 256 - k, lane 0 adds bin 128: every bin of a frame exactly once
    int n[NBIN] = {};
    for (int p = 0; p < 8; p++)
        for (int half = 0; half < 2; half++)
            for (int k2 = 0; k2 < 8; k2++) {
                n[bin(p, half, k2)]++;
                n[256 - bin(p, half, k2)]++;
            }
    n[128]++;
    for (int k = 0; k < NBIN; k++)
        if (n[k] != 1) return false;
    return true;
}
static_assert(rows_fit(), "sixteen distinct rows per pass inside the wave's eight P rows, store offsets inside the instruction's 16-bit field");
static_assert(store_byte(15, 1) / 4 + 64 <= AREA && store_byte(9, 1) / 4 + 64 == AREA, "the layout ends where the eighth P row ends");
static_assert(reads_match_stores(), "a stage-2 lane's ds_read2_b32 pairs are the two mirror columns of its frame; offset1 <= 255");
static_assert(mirrors_match(), "the untangle's partner of every bin sits in the same lane");
static_assert(bins_once(), "bins 0..256 of a frame are each produced exactly once");

}  // namespace paircol
