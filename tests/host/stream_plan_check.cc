// Stand-alone check of the push planner of a stream set (ctucopy_amd/csrc/stream_plan.h): no engine library, no GPU, no HIP.
// tests/test_stream_plan_cpu.py builds it under Address+UB sanitizers and runs it: exit status 0, a final "stream_plan_check ok"
// and a silent stderr are the result.  A few thousand random pushes, each against the restatement below, which counts frames one
// by one and follows the chains link by link.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
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

// ---- the restatement: frame t of a file is complete once the file holds the window - wshift samples loaded first and t + 1 hops
// behind them (a trailing partial window never makes a frame)
static int64_t frames_of(int64_t total, int window, int wshift) {
    int64_t F = 0;
    while ((window - wshift) + (F + 1) * wshift <= total) F++;
    return F;
}
static int64_t rows_of(int H, int wmax, int64_t F) {
    if (H == 0) return F;        // no chain: a frame's row goes out with it
    if (F < wmax + 2) return 0;  // nothing before frame wmax + 2 exists
    return F > H ? F - H : 0;
}
static int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// The arrays of a layout, owned here; `fill` is what they hold ahead of a plan
struct Arrays {
    std::vector<StreamPush> push;
    std::vector<RowPush> rows;
    std::vector<int> heads, tail;
    std::vector<int64_t> counts, consumed;
    std::vector<uint8_t> hsel;
    PushLayout L;
    Arrays(int n_streams, int max_chains, unsigned char fill) {
        const int nh = chain_deal(n_streams, max_chains).heads();
        push.resize(n_streams); rows.resize(n_streams); heads.resize(nh); tail.resize(nh);
        counts.resize(n_streams); consumed.resize(n_streams); hsel.resize(n_streams);
        std::memset(push.data(), fill, push.size() * sizeof(StreamPush));
        std::memset(rows.data(), fill, rows.size() * sizeof(RowPush));
        std::memset(heads.data(), fill, heads.size() * sizeof(int));
        std::memset(tail.data(), fill, tail.size() * sizeof(int));
        std::memset(counts.data(), fill, counts.size() * 8);
        std::memset(consumed.data(), fill, consumed.size() * 8);
        std::memset(hsel.data(), fill, hsel.size());
        L.push = push.data(); L.rows = rows.data(); L.heads = heads.data(); L.tail = tail.data();
        L.row_counts = counts.data(); L.consumed = consumed.data(); L.hsel = hsel.data();
    }
};

// everything of a layout that a launch or a commit reads, byte for byte
static bool same_layout(const PushGeom &g, int n, const Arrays &a, const Arrays &b) {
    const PushLayout &x = a.L, &y = b.L;
    if (x.n_heads != y.n_heads || x.tiles != y.tiles || x.slices != y.slices || x.grid != y.grid || x.base_rows != y.base_rows ||
        x.rows_out != y.rows_out || x.most != y.most)
        return false;
    if (std::memcmp(x.push, y.push, (size_t)n * sizeof(StreamPush))) return false;
    if (g.held && std::memcmp(x.rows, y.rows, (size_t)n * sizeof(RowPush))) return false;
    if (std::memcmp(x.heads, y.heads, (size_t)x.n_heads * sizeof(int))) return false;
    return !std::memcmp(x.row_counts, y.row_counts, (size_t)n * 8) && !std::memcmp(x.consumed, y.consumed, (size_t)n * 8) && !std::memcmp(x.hsel, y.hsel, (size_t)n);
}

static int pushes_checked = 0;

static void check_push(const PushGeom &g0, const std::vector<int64_t> &consumed, const std::vector<uint8_t> &hsel, const std::vector<int32_t> &ids,
                       const std::vector<int64_t> &ns, const std::vector<int64_t> &off, Arrays &kept) {
    const int n = (int)ids.size(), n_streams = (int)consumed.size();
    // ---- what the push must be, from the restatement
    std::vector<int64_t> F(n), T(n), len(n), slot(n), row0(n), nr(n), r0(n), out0(n);
    std::vector<int> tile0(n), live;
    int64_t so = PCM_HEAD, ro = 0, oo = 0, most = 0;
    int tiles = 0, slices = 1;
    for (int i = 0; i < n; i++) {
        const int64_t c = consumed[ids[i]];
        F[i] = frames_of(c, g0.window, g0.wshift);
        T[i] = frames_of(c + ns[i], g0.window, g0.wshift) - F[i];
        len[i] = STREAM_LEAD + (c - F[i] * g0.wshift) + ns[i];  // lead | carry | new samples
        slot[i] = so; row0[i] = ro; tile0[i] = tiles; out0[i] = oo;
        r0[i] = rows_of(g0.H, g0.wmax, F[i]);
        nr[i] = rows_of(g0.H, g0.wmax, F[i] + T[i]) - r0[i];
        so += round_up(len[i], PCM_ALIGN);
        ro += T[i];
        tiles += (int)((T[i] + TILE - 1) / TILE);
        if ((len[i] + STREAM_SLICE - 1) / STREAM_SLICE > slices) slices = (int)((len[i] + STREAM_SLICE - 1) / STREAM_SLICE);
        oo += nr[i];
        if (nr[i] > most) most = nr[i];
        if (T[i] > 0) live.push_back(i);
    }
    // ---- the plan, against an arena and a tile list that just hold it
    PushGeom g = g0;
    g.arena_samples = so + PCM_TAIL;
    g.tile_cap = tiles;
    const std::vector<int64_t> consumed_before = consumed, ns_before = ns, off_before = off;
    const std::vector<uint8_t> hsel_before = hsel;
    const std::vector<int32_t> ids_before = ids;
    Arrays fresh(n_streams, g.max_chains, 0xAB);
    const int64_t *offp = off.empty() ? nullptr : off.data();
    CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), offp, fresh.L));
    CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), offp, kept.L));  // (`kept` has held larger pushes)
    Arrays again(n_streams, g.max_chains, 0);
    CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), offp, again.L));
    CHECK(same_layout(g, n, fresh, kept));
    CHECK(same_layout(g, n, fresh, again));
    CHECK(consumed == consumed_before && hsel == hsel_before && ids == ids_before && ns == ns_before && off == off_before);
    const PushLayout &L = fresh.L;
    // slots and prefix sums
    CHECK(L.tiles == tiles && L.slices == slices && L.base_rows == ro && L.rows_out == oo && L.most == most);
    int64_t count_sum = 0;
    for (int i = 0; i < n; i++) {
        const StreamPush &p = L.push[i];
        CHECK(p.slot == slot[i] && p.slot % PCM_ALIGN == 0 && p.row0 == row0[i] && p.tile0 == tile0[i] && p.id == ids[i] && p.n == ns[i]);
        CHECK(p.src == (ns[i] ? off[i] : 0));
        CHECK(L.row_counts[i] == nr[i] && nr[i] >= 0);
        CHECK(L.consumed[i] == consumed[ids[i]] + ns[i]);
        CHECK(L.hsel[i] == (hsel[ids[i]] ^ (g.held && T[i] > 0 ? 1 : 0)));
        count_sum += L.row_counts[i];
        if (g.held) {
            const RowPush &r = L.rows[i];
            CHECK(r.F0 == F[i] && r.r0 == r0[i] && r.out0 == out0[i] && r.row0 == row0[i] && r.id == ids[i] && r.Tn == T[i] && r.nr == nr[i] &&
                  r.hsel == hsel[ids[i]]);
        }
    }
    CHECK(count_sum == L.rows_out);  // what the capacity check of a push compares against
    // chains
    if (!g.chained) {
        CHECK(L.n_heads == 0);
        CHECK(L.grid == std::max(1, std::min(tiles, g.max_wg)));
        for (int i = 0; i < n; i++) CHECK(L.push[i].pad == -1);
    } else {
        const int C = std::max(1, std::min((int)live.size(), g.max_chains)), G = (C + NWAVE - 1) / NWAVE;
        CHECK(L.grid == G && L.n_heads == G * NWAVE);
        std::map<int, int> by_tile;  // the live stream whose first tile this is
        for (int i : live) by_tile[tile0[i]] = i;
        std::vector<int> visits(n, 0);
        std::vector<char> is_head((size_t)G * NWAVE, 0);
        for (int c = 0; c < C; c++) {
            const int s = (c % G) * NWAVE + c / G;
            CHECK(s >= 0 && s < L.n_heads && !is_head[s]);
            is_head[s] = 1;
            std::vector<int> walked;
            for (int t = L.heads[s]; t >= 0 && (int)walked.size() <= n;) {
                const auto it = by_tile.find(t);
                CHECK(it != by_tile.end());
                if (it == by_tile.end()) break;
                walked.push_back(it->second);
                visits[it->second]++;
                t = L.push[it->second].pad;
            }
            std::vector<int> want;  // live stream j, in push order, is on chain j % C
            for (size_t j = (size_t)c; j < live.size(); j += (size_t)C) want.push_back(live[j]);
            CHECK(walked == want);
        }
        for (int s = 0; s < L.n_heads; s++)
            if (!is_head[s]) CHECK(L.heads[s] == -1);
        for (int i = 0; i < n; i++) {
            CHECK(visits[i] == (T[i] > 0 ? 1 : 0));
            if (T[i] == 0) CHECK(L.push[i].pad == -1);
        }
    }
    // one unit too small: the error, and the caller's mirrors as they were
    PushGeom tight = g;
    tight.arena_samples = g.arena_samples - 1;
    CHECK(!stream_plan_push(tight, consumed.data(), hsel.data(), n, ids.data(), ns.data(), offp, again.L));
    if (tiles > 0) {
        tight = g;
        tight.tile_cap = tiles - 1;
        CHECK(!stream_plan_push(tight, consumed.data(), hsel.data(), n, ids.data(), ns.data(), offp, again.L));
    }
    CHECK(consumed == consumed_before && hsel == hsel_before);
    pushes_checked++;
}

static void check_finish(int window, int wshift, int H, int wmax) {
    for (int64_t F = 0; F <= wmax + 3; F++)
        for (int64_t extra : {(int64_t)0, (int64_t)1, (int64_t)wshift - 1}) {
            const int64_t total = F == 0 && extra == 0 ? 0 : (window - wshift) + F * wshift + extra;
            if (frames_of(total, window, wshift) != F) continue;  // (wshift == 1: the extra sample is a frame)
            const FinishLayout f = stream_plan_finish(window, wshift, H, wmax, total, 5, 1);
            const bool too_short = H > 0 && F > 0 && F < wmax + 2;
            const int64_t pending = F - rows_of(H, wmax, F);  // ctu_streams_rows_step's
            CHECK(f.frames == F && f.too_short == too_short);
            CHECK(f.pending == (too_short ? 0 : pending));
            if (f.pending > 0) CHECK(f.row.F0 == F && f.row.r0 == F - pending && f.row.out0 == 0 && f.row.row0 == 0 && f.row.id == 5 && f.row.Tn == 0 &&
                                     f.row.nr == pending && f.row.hsel == 1);
        }
}

int main() {
    std::mt19937 rng(20240611u);
    auto below = [&](int64_t m) { return (int64_t)(rng() % (uint64_t)m); };
    const int win[3][2] = {{400, 160}, {200, 80}, {400, 161}};
    const int halo[4][2] = {{0, 0}, {4, 2}, {6, 3}, {3, 3}};  // (the last: a stacking, whose halo is its window)
    for (const auto &ws : win)
        for (const auto &hw : halo) {
            check_finish(ws[0], ws[1], hw[0], hw[1]);
            for (int max_chains : {1, 3, 8, 17})
                for (int max_wg : {1, 2, 5})
                    for (int chained = 0; chained < 2; chained++) {
                        const int n_streams = 1 + (int)below(40);
                        const int64_t max_push = 1 + below(3 * TILE * ws[1]);  // up to three tiles, and past one slice
                        PushGeom g{};
                        g.window = ws[0]; g.wshift = ws[1]; g.H = hw[0]; g.wmax = hw[1];
                        g.held = hw[0] > 0 || below(2) == 1;  // (CMS alone holds rows without a halo)
                        g.chained = chained != 0; g.max_chains = max_chains; g.max_wg = max_wg;
                        std::vector<int64_t> consumed((size_t)n_streams, 0);
                        std::vector<uint8_t> hsel((size_t)n_streams, 0);
                        Arrays kept(n_streams, max_chains, 0xCD);
                        std::vector<int32_t> order((size_t)n_streams);
                        for (int round = 0; round < 14; round++) {
                            for (int i = 0; i < n_streams; i++) order[(size_t)i] = i;
                            std::shuffle(order.begin(), order.end(), rng);
                            const int n = round == 0 ? n_streams : 1 + (int)below(n_streams);  // (the first push is the largest: `kept` holds it)
                            std::vector<int32_t> ids(order.begin(), order.begin() + n);
                            std::vector<int64_t> ns((size_t)n), off((size_t)n);
                            int64_t at = 0;
                            for (int i = 0; i < n; i++) {
                                const int64_t c = consumed[(size_t)ids[i]];
                                const int64_t next = (g.window - g.wshift) + (frames_of(c, g.window, g.wshift) + 1) * g.wshift;  // samples at the next frame
                                int64_t v = 0;
                                switch (below(6)) {
                                    case 0: v = 0; break;
                                    case 1: v = 1; break;
                                    case 2: v = next - 1 - c; break;                         // just short of a frame
                                    case 3: v = next - c; break;                             // exactly one
                                    case 4: v = next - c + (TILE - 1) * g.wshift + below(2); break;  // a full tile, or one sample into the next frame
                                    default: v = below(max_push + 1); break;
                                }
                                ns[(size_t)i] = std::max<int64_t>(0, std::min(v, max_push));
                                off[(size_t)i] = at;
                                at += ns[(size_t)i] + below(3);
                            }
                            check_push(g, consumed, hsel, ids, ns, off, kept);
                            // the commit
                            Arrays plan(n_streams, max_chains, 0);
                            PushGeom roomy = g;
                            roomy.arena_samples = roomy.tile_cap = INT64_MAX / 2;
                            CHECK(stream_plan_push(roomy, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), plan.L));
                            for (int i = 0; i < n; i++) {
                                consumed[(size_t)ids[i]] = plan.L.consumed[i];
                                hsel[(size_t)ids[i]] = plan.L.hsel[i];
                            }
                            if (below(4) == 0) consumed[(size_t)below(n_streams)] = 0;  // a stream finishes now and then
                        }
                    }
        }
    if (failures) {
        std::printf("stream_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_plan_check ok (%d pushes)\n", pushes_checked);
    return 0;
}
