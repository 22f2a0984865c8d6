// Stand-alone check of the push planner's trap geometry (ctucopy_amd/csrc/stream_plan.h: stream_trap_halo, stream_trap_columns): no
// engine library, no GPU, no HIP.  tests/test_streams_trap_cpu.py builds it under Address+UB sanitizers and runs it: exit status 0, a
// final "stream_trap_plan_check ok" and a silent stderr are the result.  Sets of streams are driven through a few thousand random
// pushes and finishes, with the mirrors committed as ctu_streams_push commits them.  Every push is checked against a restatement that
// walks the frames one by one - frame f of a file completes row f - half once f >= half - and then walks stream_trap_kernel's columns
// as the kernel does: the stream of every column from the table, its row, and every log-mel frame its taps name behind the kernel's
// clamps, which must be a fresh row of the push or a row the history holds, and the very frame the offline formula names.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "stream_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static int64_t frames_of(int64_t total, int window, int wshift) {
    int64_t F = 0;
    while ((window - wshift) + (F + 1) * wshift <= total) F++;
    return F;
}

static int pushes_checked = 0, finishes_checked = 0, short_files = 0, shared_groups = 0, three_stream_groups = 0, big_pushes = 0;
static int64_t columns_checked = 0;

// One column as stream_trap_kernel walks it: row t = r0 + (c - out0) of the stream, taps 0 .. 4 ceil(traplen / 4) - 1.  `T`: the file's
// length where it is known (a finish), else -1.  `hist_lo`: the oldest frame the history at hand holds (F0 - C, or 0).
static void check_column(const RowPush &r, int64_t c, int traplen, int C, int64_t base_rows, int64_t T) {
    const int half = (traplen - 1) / 2, nsteps = (traplen + 3) / 4;
    const int64_t t = r.r0 + (c - r.out0);
    const int trel = (int)(t - r.F0), lo = -(int)std::min<int64_t>(r.F0, C), hi = r.Tn - 1;
    CHECK(lo <= hi && trel >= lo && trel <= hi);  // the column's own centre frame exists and is in reach
    for (int j = 0; j < 4 * nsteps; j++) {
        const int rel = std::min(std::max(trel - half + j, lo), hi);
        // where the kernel reads: a fresh row of the push, or a row of the history
        if (rel >= 0) CHECK(r.row0 + rel < base_rows && rel < r.Tn);
        else CHECK(C + rel >= 0 && C + rel < C && r.F0 + rel >= 0);
        if (j < traplen) {  // a real tap: the frame of the offline formula, clamp(t - half + j, 0, T - 1)
            int64_t f = t - half + j;
            f = f < 0 ? 0 : f;
            if (T >= 0) f = std::min(f, T - 1);
            else CHECK(f <= r.F0 + r.Tn - 1);  // mid-stream a row goes out only when every frame it reads exists
            CHECK(r.F0 + rel == f);
        }
    }
    columns_checked++;
}

static void run_set(int window, int wshift, int traplen, bool chained, int n_streams, unsigned seed) {
    std::mt19937 rng(seed);
    const int half = (traplen - 1) / 2, C = 2 * half;
    PushGeom g{};
    g.window = window; g.wshift = wshift;
    stream_trap_halo(traplen, &g.H, &g.wmax);
    CHECK(g.H == half && g.wmax == half - 1);
    g.held = true;
    g.chained = chained;
    g.max_chains = 5; g.max_wg = 3;
    g.arena_samples = INT64_MAX / 4; g.tile_cap = 1 << 30;
    const int nh = chain_deal(n_streams, g.max_chains).heads();
    std::vector<StreamPush> push(n_streams);
    std::vector<RowPush> rows(n_streams);
    std::vector<int> heads(nh), tail(nh);
    std::vector<int64_t> counts(n_streams), next_consumed(n_streams), consumed(n_streams, 0), delivered(n_streams, 0);
    std::vector<uint8_t> next_hsel(n_streams), hsel(n_streams, 0);
    const int max_push = window + (3 * half + 5) * wshift;  // more frames in one push than the history holds
    for (int round = 0; round < 120; round++) {
        // ---- a push of some of the streams, in a shuffled order
        std::vector<int32_t> ids;
        for (int s = 0; s < n_streams; s++)
            if (rng() % 3) ids.push_back(s);
        std::shuffle(ids.begin(), ids.end(), rng);
        const int n = (int)ids.size();
        std::vector<int64_t> ns(n), off(n);
        for (int i = 0; i < n; i++) {
            const unsigned kind = rng() % 10;
            ns[i] = kind == 0 ? 0 : kind == 1 ? (int64_t)(rng() % wshift) : kind == 2 ? max_push : kind < 6 ? wshift : (int64_t)(rng() % (5 * wshift));
            off[i] = 1000 * i;
        }
        std::memset(rows.data(), 0x5A, rows.size() * sizeof(RowPush));
        PushLayout L;
        L.push = push.data(); L.rows = rows.data(); L.heads = heads.data(); L.tail = tail.data();
        L.row_counts = counts.data(); L.consumed = next_consumed.data(); L.hsel = next_hsel.data();
        CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), L));
        // ---- the restatement of the counts, frame by frame
        int64_t oo = 0, ro = 0;
        for (int i = 0; i < n; i++) {
            const int64_t c = consumed[ids[i]];
            const int64_t F0 = frames_of(c, window, wshift), T = frames_of(c + ns[i], window, wshift) - F0;
            int64_t nr = 0;
            for (int64_t f = F0; f < F0 + T; f++) nr += f >= half;  // frame f completes row f - half
            const RowPush &r = L.rows[i];
            CHECK(r.F0 == F0 && r.Tn == T && r.r0 == delivered[ids[i]] && r.nr == nr && r.out0 == oo && r.row0 == ro && r.id == ids[i] && r.hsel == hsel[ids[i]]);
            CHECK(r.r0 == (F0 > half ? F0 - half : 0) && nr <= T);  // a push delivers at most as many rows as it completes frames
            CHECK(L.row_counts[i] == nr && L.consumed[i] == c + ns[i] && L.hsel[i] == (hsel[ids[i]] ^ (T > 0 ? 1 : 0)));
            oo += nr;
            ro += T;
            big_pushes += T > C;
            // the carry: the last C frames of the file behind this push are fresh or in the history at hand
            if (T > 0)
                for (int j = 0; j < C; j++) {
                    const int64_t f = F0 + T - C + j;
                    if (f >= 0 && f < F0) CHECK(f - F0 + C >= 0 && f - F0 + C < C);
                }
        }
        CHECK(L.rows_out == oo && L.base_rows == ro);
        // ---- the columns: the table against a search of its own, every column once, and the kernel's walk over each
        std::vector<int> col((size_t)oo + 8, 0x5A5A5A5A);
        CHECK(stream_trap_columns(L.rows, n, col.data()) == oo);
        for (int64_t c = oo; c < oo + 8; c++) CHECK(col[(size_t)c] == 0x5A5A5A5A);  // nothing past the last column
        for (int64_t c = 0; c < oo; c++) {
            int owner = -1, owners = 0;
            for (int i = 0; i < n; i++)
                if (c >= L.rows[i].out0 && c < L.rows[i].out0 + L.rows[i].nr) {
                    owner = i;
                    owners++;
                }
            CHECK(owners == 1 && col[(size_t)c] == owner);
            if (owners == 1) check_column(L.rows[owner], c, traplen, C, L.base_rows, -1);
        }
        for (int64_t c0 = 0; c0 < oo; c0 += 16) {  // how many streams the column groups of a wave hold
            int streams = 1;
            for (int64_t c = c0 + 1; c < std::min<int64_t>(c0 + 16, oo); c++) streams += col[(size_t)c] != col[(size_t)c - 1];
            shared_groups += streams > 1;
            three_stream_groups += streams > 2;
        }
        // ---- commit, as ctu_streams_push does
        for (int i = 0; i < n; i++) {
            consumed[ids[i]] = L.consumed[i];
            hsel[ids[i]] = L.hsel[i];
            delivered[ids[i]] += L.row_counts[i];
        }
        pushes_checked++;
        // ---- now and then a stream's file ends
        for (int s = 0; s < n_streams; s++)
            if (rng() % 13 == 0) {
                const int64_t F = frames_of(consumed[s], window, wshift);
                const FinishLayout f = stream_plan_finish(window, wshift, g.H, g.wmax, consumed[s], s, hsel[s]);
                CHECK(f.frames == F && f.too_short == (F > 0 && F <= half));  // a file of 1 .. half frames: the offline plan's refusal
                CHECK(f.pending == (F > half ? half : 0));
                if (!f.too_short) CHECK(delivered[s] + f.pending == F);
                if (f.pending) {
                    CHECK(f.row.F0 == F && f.row.r0 == F - half && f.row.nr == half && f.row.Tn == 0 && f.row.id == s && f.row.hsel == hsel[s] && f.row.out0 == 0);
                    std::vector<int> fc((size_t)half, -1);
                    CHECK(stream_trap_columns(&f.row, 1, fc.data()) == half);
                    for (int c = 0; c < half; c++) {
                        CHECK(fc[(size_t)c] == 0);
                        check_column(f.row, c, traplen, C, 0, F);
                    }
                }
                short_files += f.too_short;
                consumed[s] = 0;
                delivered[s] = 0;
                finishes_checked++;
            }
    }
}

int main() {
    unsigned seed = 1;
    for (int traplen : {3, 5, 31, 101, 255})
        for (int chained = 0; chained < 2; chained++) {
            run_set(200, 80, traplen, chained != 0, 9, seed++);
            run_set(400, 160, traplen, chained != 0, 37, seed++);
            run_set(64, 64, traplen, chained != 0, 3, seed++);  // no overlap: -s equal to -w
        }
    // R(F) in closed form is stream_rows_out on the halo stream_trap_halo gives: F - half once F >= half + 1 (plan.cc: trap_min), none before
    for (int traplen = 3; traplen <= 255; traplen += 2) {
        int H = 0, wmax = 0;
        stream_trap_halo(traplen, &H, &wmax);
        const int half = (traplen - 1) / 2;
        CHECK(half + 1 == (traplen + 1) / 2);
        for (int64_t F = 0; F < 300; F++) CHECK(stream_rows_out(H, wmax, F) == (F >= half + 1 ? F - half : 0));
    }
    CHECK(short_files > 5 && shared_groups > 100 && three_stream_groups > 20 && big_pushes > 20);
    if (failures) {
        std::printf("stream_trap_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_trap_plan_check ok: %d pushes, %d finishes (%d of no more than half a context), %lld columns, %d column groups over several streams (%d over three or more)\n",
                pushes_checked, finishes_checked, short_files, (long long)columns_checked, shared_groups, three_stream_groups);
    return 0;
}
