// Stand-alone check of the push planner's VAD geometry (ctucopy_amd/csrc/stream_plan.h with PushGeom::vad): no engine library, no GPU,
// no HIP.  tests/test_streams_vad_cpu.py builds it under Address+UB sanitizers and runs it: exit status 0, a final
// "stream_vad_plan_check ok" and a silent stderr are the result.  Sets of streams are driven through a few thousand random pushes and
// finishes, with the mirrors committed as ctu_streams_push commits them; every push is checked against a restatement that walks the
// frames one by one, as the detector's replay does: frame t of a file emits the byte of row t - h once t >= h.
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

static int pushes_checked = 0, finishes_checked = 0, held_files = 0, short_files = 0;

static void run_set(int window, int wshift, int order, bool chained, int n_streams, unsigned seed) {
    std::mt19937 rng(seed);
    const int h = (order - 1) / 2;
    PushGeom g{};
    g.window = window; g.wshift = wshift;
    stream_vad_halo(order, &g.H, &g.wmax);
    CHECK(g.H == h && g.wmax == (h > 0 ? h - 1 : 0));
    g.held = g.H > 0;
    g.vad = true;
    g.chained = chained;
    g.max_chains = 5; g.max_wg = 3;
    g.arena_samples = INT64_MAX / 4; g.tile_cap = 1 << 30;
    const int nh = chain_deal(n_streams, g.max_chains).heads();
    std::vector<StreamPush> push(n_streams);
    std::vector<RowPush> rows(n_streams);
    std::vector<int> heads(nh), tail(nh), replay(n_streams);
    std::vector<int64_t> counts(n_streams), next_consumed(n_streams), consumed(n_streams, 0), delivered(n_streams, 0);
    std::vector<uint8_t> next_hsel(n_streams), hsel(n_streams, 0);
    const int max_push = window + 70 * wshift;  // two tiles and more in one push
    for (int round = 0; round < 160; round++) {
        // ---- a push of some of the streams, in a shuffled order
        std::vector<int32_t> ids;
        for (int s = 0; s < n_streams; s++)
            if (rng() % 3) ids.push_back(s);
        std::shuffle(ids.begin(), ids.end(), rng);
        const int n = (int)ids.size();
        std::vector<int64_t> ns(n), off(n);
        for (int i = 0; i < n; i++) {
            const unsigned kind = rng() % 8;
            ns[i] = kind == 0 ? 0 : kind == 1 ? (int64_t)(rng() % wshift) : kind == 2 ? max_push : (int64_t)(rng() % (9 * wshift));
            off[i] = 1000 * i;
        }
        std::memset(replay.data(), 0x5A, replay.size() * sizeof(int));
        std::memset(rows.data(), 0x5A, rows.size() * sizeof(RowPush));
        PushLayout L;
        L.push = push.data(); L.rows = rows.data(); L.heads = heads.data(); L.tail = tail.data(); L.replay = replay.data();
        L.row_counts = counts.data(); L.consumed = next_consumed.data(); L.hsel = next_hsel.data();
        CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), L));
        // ---- the restatement
        std::vector<unsigned char> byte_written((size_t)L.rows_out, 0);
        int64_t oo = 0, ro = 0, most = 0;
        int n_replay = 0;
        for (int i = 0; i < n; i++) {
            const int64_t c = consumed[ids[i]];
            const int64_t F0 = frames_of(c, window, wshift), T = frames_of(c + ns[i], window, wshift) - F0;
            const int64_t r0 = F0 > h ? F0 - h : 0, r1 = F0 + T > h ? F0 + T - h : 0;
            const RowPush &r = L.rows[i];
            CHECK(r.F0 == F0 && r.Tn == T && r.r0 == r0 && r.nr == r1 - r0 && r.out0 == oo && r.row0 == ro && r.id == ids[i] && r.hsel == hsel[ids[i]]);
            CHECK(L.row_counts[i] == r1 - r0 && L.consumed[i] == c + ns[i]);
            CHECK(L.hsel[i] == (hsel[ids[i]] ^ (h > 0 && T > 0 ? 1 : 0)));
            CHECK(r0 == delivered[ids[i]]);  // what the host mirrors is what has gone out
            if (T > 0) {
                CHECK(n_replay < L.n_replay && L.replay[n_replay] == i);  // the replay's streams: those that complete a frame, in push order
                n_replay++;
            }
            // the replay, frame by frame: where every byte goes, and that each byte of the push is written once and inside the push
            for (int64_t t = F0; t < F0 + T; t++)
                if (t >= h) {
                    const int64_t at = r.out0 + (t - h) - r.r0;
                    CHECK(at >= 0 && at < L.rows_out);
                    if (at >= 0 && at < L.rows_out) {
                        CHECK(!byte_written[(size_t)at]);
                        byte_written[(size_t)at] = 1;
                    }
                }
            // the delayed copy: every row that goes out is a fresh base row of the push or one of the h the history holds
            for (int64_t row = r0; row < r1; row++) {
                if (row >= F0) CHECK(r.row0 + (row - F0) < L.base_rows && row - F0 < T);
                else CHECK(row - F0 + h >= 0 && row - F0 + h < h);
            }
            // the carry: the last h frames of the file behind this push are fresh or in the history at hand
            if (T > 0)
                for (int j = 0; j < h; j++) {
                    const int64_t f = F0 + T - h + j;
                    if (f >= 0 && f < F0) CHECK(f - F0 + h >= 0 && f - F0 + h < h);
                }
            oo += r1 - r0;
            ro += T;
            if (r1 - r0 > most) most = r1 - r0;
        }
        CHECK(n_replay == L.n_replay && L.rows_out == oo && L.base_rows == ro && L.most == most);
        for (unsigned char b : byte_written) CHECK(b == 1);
        for (int i = L.n_replay; i < n_streams; i++) CHECK(replay[i] == 0x5A5A5A5A);  // entries past the list are left alone
        // ---- commit, as ctu_streams_push does
        for (int i = 0; i < n; i++) {
            consumed[ids[i]] = L.consumed[i];
            hsel[ids[i]] = L.hsel[i];
            delivered[ids[i]] += L.row_counts[i];
        }
        pushes_checked++;
        // ---- now and then a stream's file ends
        for (int s = 0; s < n_streams; s++)
            if (rng() % 11 == 0) {
                const int64_t F = frames_of(consumed[s], window, wshift);
                const FinishLayout f = stream_plan_finish(window, wshift, g.H, g.wmax, consumed[s], s, hsel[s], true);
                CHECK(f.frames == F && !f.too_short);
                CHECK(f.pending == (F > h ? h : 0));
                CHECK(delivered[s] + f.pending == (F > h ? F : 0));  // a file of no more than h frames writes nothing
                if (f.pending) CHECK(f.row.F0 == F && f.row.r0 == F - h && f.row.nr == h && f.row.Tn == 0 && f.row.id == s && f.row.hsel == hsel[s] && f.row.out0 == 0);
                // without the flag's rule the same file is the chain's refusal
                const FinishLayout plain = stream_plan_finish(window, wshift, g.H, g.wmax, consumed[s], s, hsel[s]);
                CHECK(plain.too_short == (h > 0 && F > 0 && F <= h) && plain.pending == f.pending);
                held_files += f.pending > 0;
                short_files += h > 0 && F > 0 && F <= h;
                consumed[s] = 0;
                delivered[s] = 0;
                finishes_checked++;
            }
    }
}

int main() {
    unsigned seed = 1;
    for (int order : {1, 2, 3, 5, 7, 31})
        for (int chained = 0; chained < 2; chained++) {
            run_set(200, 80, order, chained != 0, 9, seed++);
            run_set(400, 160, order, chained != 0, 37, seed++);
            run_set(64, 64, order, chained != 0, 3, seed++);  // no overlap: -s equal to -w
        }
    // R(F) in closed form is stream_rows_out on the halo stream_vad_halo gives
    for (int order = 1; order <= 31; order++) {
        int H = 0, wmax = 0;
        stream_vad_halo(order, &H, &wmax);
        for (int64_t F = 0; F < 80; F++) CHECK(stream_rows_out(H, wmax, F) == (F > H ? F - H : 0));
    }
    CHECK(held_files > 50 && short_files > 5);
    if (failures) {
        std::printf("stream_vad_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_vad_plan_check ok: %d pushes, %d finishes (%d with held rows, %d of no more than h frames)\n", pushes_checked, finishes_checked,
                held_files, short_files);
    return 0;
}
