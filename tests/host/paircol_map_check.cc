// The index maps of the pair-column second stage (ctucopy_amd/csrc/paircol_map.h), checked by enumeration in a program of its own
// (tests/test_paircol_map_cpu.py builds it under Address+UB sanitizers and runs it directly).
//
// It plays a step through a model of the wave's eight P rows: stage 1 stores element (k1, pass, fg, n2) where the add-TID stores put
// it, stage 2 reads what its ds_read2_b32 pairs address, and the untangle must then find, for every bin of every frame, its mirror
// bin in the same lane - lane p = 0 included - and the twiddle record of the bin's own column.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "paircol_map.h"

namespace pc = paircol;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
            failures++;                        \
        }                                      \
    } while (0)

// an element's identity: which value of the step it is
static int ident(int k1, int pass, int fg, int n2) { return ((k1 * 2 + pass) * 4 + fg) * 16 + n2 + 1; }

// LDS cycles of one read instruction over a half wave under the host model (32 lanes per cycle, 32 banks, one dword per bank and cycle;
// lanes that read the same dword share a cycle)
static int read_cycles(const std::vector<int> &dwords) {
    int worst = 0;
    for (int bank = 0; bank < 32; bank++) {
        std::set<int> distinct;
        for (int a : dwords)
            if (a % 32 == bank) distinct.insert(a);
        if ((int)distinct.size() > worst) worst = (int)distinct.size();
    }
    return worst;
}

int main() {
    // ---- the layout: stores land inside the area, on cells of their own; reads return the frame's two mirror columns
    std::vector<int> area(pc::AREA, 0);
    for (int k1 = 0; k1 < 16; k1++)
        for (int pass = 0; pass < 2; pass++) {
            const int byte = pc::store_byte(k1, pass);
            CHECK(byte >= 0 && byte % 4 == 0 && byte + 4 * 63 < 65536, "store offset of row %d pass %d out of the instruction's range: %d", k1, pass, byte);
            for (int lane = 0; lane < 64; lane++) {  // stage-1 lane = 16 fg + n2
                const int at = byte / 4 + lane;
                CHECK(at < pc::AREA, "row %d pass %d leaves the wave's eight P rows: dword %d", k1, pass, at);
                if (at >= pc::AREA) continue;
                CHECK(area[at] == 0, "dword %d is written twice", at);
                area[at] = ident(k1, pass, lane >> 4, lane & 15);
            }
        }
    CHECK(pc::D + 15 <= 255, "offset1 = D + n2 exceeds the 8-bit field");
    int v[64][2][16];  // stage-2 input: [lane][half][n2]
    for (int lane = 0; lane < 64; lane++) {
        const int f8 = pc::lane_f8(lane), p = pc::lane_p(lane);
        CHECK(f8 >= 0 && f8 < 8 && p >= 0 && p < 8 && pc::lane_of(f8, p) == lane, "lane %d <-> (f8 %d, p %d) is no bijection", lane, f8, p);
        for (int half = 0; half < 2; half++)
            for (int n2 = 0; n2 < 16; n2++) {
                const int at = pc::read_dword(lane) + half * pc::D + n2;
                CHECK(at >= 0 && at < pc::AREA, "lane %d reads outside the area: dword %d", lane, at);
                v[lane][half][n2] = (at >= 0 && at < pc::AREA) ? area[at] : 0;
                CHECK(v[lane][half][n2] == ident(pc::column(p, half), f8 >> 2, f8 & 3, n2), "lane %d half %d n2 %d reads the wrong element", lane, half, n2);
            }
    }
    // every column of every frame is in exactly one (lane, half)
    for (int f8 = 0; f8 < 8; f8++) {
        int seen[16] = {0};
        for (int p = 0; p < 8; p++)
            for (int half = 0; half < 2; half++) seen[pc::column(p, half)]++;
        for (int c = 0; c < 16; c++) CHECK(seen[c] == 1, "column %d of frame %d is held %d times", c, f8, seen[c]);
    }

    // ---- the untangle: after the second DFT register r of (lane p, half) is Z[column + 16 r], all 16 x 16 elements of a frame
    int produced[pc::NBIN] = {0};
    for (int c = 0; c < 16; c++)
        for (int r = 0; r < 16; r++) {
            const int k = c + 16 * r, mk = (256 - k) % 256;  // the element's bin, its mirror's bin
            int p = -1, half = -1;
            for (int pp = 0; pp < 8; pp++)
                for (int h = 0; h < 2; h++)
                    if (pc::column(pp, h) == c) p = pp, half = h;
            CHECK(p >= 0, "column %d is in no lane", c);
            if (p < 0) continue;
            if (r < 8) {  // the element is the `a` operand of step k2 = r
                CHECK(pc::bin(p, half, r) == k, "bin of (column %d, register %d)", c, r);
                const int mh = pc::mirror_half(p, half), mr = pc::mirror_reg(p, half, r);
                CHECK(mr >= 0 && mr < 16 && pc::column(p, mh) + 16 * mr == mk, "mirror of (column %d, register %d): (column %d, register %d), bin %d wanted", c, r, pc::column(p, mh), mr, mk);
                CHECK(pc::twiddle_record(p, half) == c && pc::twiddle_record(p, half) + 16 * r == k, "twiddle record of (column %d, register %d)", c, r);
                produced[k]++;
                produced[256 - k]++;
            } else if (!(c == 0 && r == 8)) {  // the element is the partner operand of exactly one step
                int uses = 0;
                for (int h = 0; h < 2; h++)
                    for (int k2 = 0; k2 < 8; k2++)
                        if (pc::mirror_half(p, h) == half && pc::mirror_reg(p, h, k2) == r) uses++;
                CHECK(uses == 1, "(column %d, register %d) is the partner of %d steps", c, r, uses);
            }
        }
    produced[128]++;  // column 0, register 8: its own mirror, written by lane p = 0
    CHECK(pc::column(0, 0) == 0, "bin 128 comes from lane p = 0's low half");
    for (int k = 0; k < pc::NBIN; k++) CHECK(produced[k] == 1, "bin %d is produced %d times", k, produced[k]);

    // ---- bank conflicts of the transposed reads, against the layout this one replaces (rows 129 dwords apart, pass B at + 64,
    // lane (k1 = lane & 15, fg = lane >> 4) reading 129 k1 + 16 fg + n2 and 64 more)
    int cycles_new = 0, cycles_old = 0;
    for (int hw = 0; hw < 2; hw++)
        for (int n2 = 0; n2 < 16; n2++)
            for (int second = 0; second < 2; second++) {
                std::vector<int> a_new, a_old;
                for (int lane = 32 * hw; lane < 32 * hw + 32; lane++) {
                    a_new.push_back(pc::read_dword(lane) + second * pc::D + n2);
                    a_old.push_back(129 * (lane & 15) + 16 * (lane >> 4) + second * 64 + n2);
                }
                const int cn = read_cycles(a_new), co = read_cycles(a_old);
                CHECK(cn == 1, "half wave %d, n2 %d, offset%d: %d cycles (32 distinct banks wanted)", hw, n2, second, cn);
                cycles_new += cn;
                cycles_old += co;
            }
    CHECK(cycles_new <= cycles_old, "transposed reads: %d LDS cycles against the replaced layout's %d", cycles_new, cycles_old);

    if (failures) {
        std::fprintf(stderr, "paircol_map_check: %d failures\n", failures);
        return 1;
    }
    std::printf("paircol_map_check ok: reads %d cycles, replaced layout %d\n", cycles_new, cycles_old);
    return 0;
}
