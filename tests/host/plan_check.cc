// Stand-alone walk over the planner of an offline run (ctucopy_amd/csrc/plan.cc with tables.cc, accept.cc, opts.cc and design.cc): no
// engine library, no GPU, no HIP.  tests/test_host_plans.py builds it under Address+UB sanitizers and runs it on the cases of
// tests/golden/host_plans.json: exit status 0, a silent stderr and the golden file's hashes and refusal texts are the result.
//
// Input (argv[1]), a line per case, tab-separated:  kind  name  n_cu  lengths  aux  arg...   (lists comma-separated, "-" = empty)
//   kind P: build_host_plan                                    -> P name <words> <sha256>, or R name <code> <text in hex> when refused
//   kind G: plan_ring_src / vad_ring_step / vad_ring_rows with the filter order and the start indices `aux` = order,hidx...
//   kind S: plan_part_first with `aux` = nparts                 -> as P
// A report is 64-bit words, hashed as little-endian int64.  Kind P, every list preceded by its count: n_utt, total_samples,
// total_frames, n_tiles, grid, max_frames, n_live | nsamples | sample_off | row_off | frames | tiles (sbase, rbase, nvalid, t0, next, T
// each) | heads | uinfo (four ints each) | n_chunks, chunks | n_chunks128, chunks128 | tile_utt | vf_order | out_samples | the device
// image of sample_off (empty unless PlanScratch::d_sample_off) | that of row_off | the PlanScratch counts: base_rows, d_sample_off,
// d_row_off, ss_seed, ss_last, ss_dirty, ss_vbits, xri, pnr, pss, vad_ci, vad_cf, ybuf, dc1m, dc1, logmel, lp_r.  Kind G: the ring
// sources of the plan, then per utterance the index and size vad_ring_step leaves from (hidx, 0), what vad_ring_rows returns and that
// many source frames.  Kind S: the first utterance of every range.
//
// Every plan over samples is also checked for what the kernels trust, record or no record (a breach is reported on stderr):
// every tile is on exactly one chain; under per_wave a chain holds whole utterances in tile order; no chain's load exceeds the
// lightest chain's by more than the longest utterance.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "accept.h"
#include "check_digest.h"
#include "plan_host.h"
#include "tables.h"

using namespace ctu;
typedef std::vector<int64_t> Words;

template <class T>
static void put(Words &v, const std::vector<T> &list) {
    v.push_back((int64_t)list.size());
    for (const T &x : list) v.push_back((int64_t)x);
}

static Words plan_report(const HostPlan &p) {
    const PlanScratch &s = p.scratch;
    Words v = {p.n_utt, p.total_samples, p.total_frames, (int64_t)p.tiles.size(), p.grid, p.max_frames, p.n_live};
    put(v, p.nsamples);
    put(v, p.sample_off);
    put(v, p.row_off);
    put(v, p.frames);
    v.push_back((int64_t)p.tiles.size());
    for (const TileRec &t : p.tiles) v.insert(v.end(), {t.sbase, t.rbase, t.nvalid, t.t0, t.next, t.T});
    put(v, p.heads);
    v.push_back((int64_t)p.uinfo.size() * 4);
    for (const UttInfo &u : p.uinfo) v.insert(v.end(), {u.row_lo, u.row_hi, u.frames, u.pad});
    v.push_back(p.n_chunks);
    put(v, p.chunks);
    v.push_back(p.n_chunks128);
    put(v, p.chunks128);
    put(v, p.tile_utt);
    put(v, p.vf_order);
    put(v, p.out_samples);
    put(v, s.d_sample_off ? p.sample_off : std::vector<int64_t>());
    put(v, s.d_row_off ? p.row_off : std::vector<int64_t>());
    v.insert(v.end(), {s.base_rows, s.d_sample_off, s.d_row_off, s.ss_seed, s.ss_last, s.ss_dirty, s.ss_vbits, s.xri, s.pnr, s.pss, s.vad_ci, s.vad_cf, s.ybuf, s.dc1m,
                       s.dc1, s.logmel, s.lp_r});
    return v;
}

// What the kernels trust of the chains; "" when it holds.
static std::string chains_breach(const PlanGeom &g, const HostPlan &p) {
    const int n_tiles = (int)p.tiles.size();
    if (p.uts.size() != (size_t)p.n_utt + 1 || p.uts.back() != n_tiles) return "first tiles of the utterances";
    std::vector<int> utt_of(n_tiles, -1), seen(n_tiles, 0);
    for (int u = 0; u < p.n_utt; u++)
        for (int t = p.uts[u]; t < p.uts[u + 1]; t++) utt_of[t] = u;
    int64_t longest = 0, lightest = INT64_MAX, heaviest = 0;
    for (int64_t f : p.frames) longest = std::max(longest, f);
    for (int head : p.heads) {
        if (head < -1 || head >= n_tiles) return "a chain head outside the tile list";
        int64_t load = 0;
        for (int t = head, steps = 0; t >= 0; t = p.tiles[t].next, steps++) {
            if (t >= n_tiles || steps > n_tiles) return "a tile's next outside the tile list, or a cycle";
            if (seen[t]++) return "a tile on two chains";
            load += p.tiles[t].nvalid;
            if (g.per_wave) {  // whole utterances, tile after tile: a chain enters an utterance at its first tile and leaves it behind its last
                const int u = utt_of[t], nx = p.tiles[t].next;
                const bool first = t == p.uts[u], last = t == p.uts[u + 1] - 1;
                if ((t == head && !first) || (!last && nx != t + 1) || (last && nx >= 0 && nx != p.uts[utt_of[nx]])) return "a chain that holds part of an utterance";
            }
        }
        if (head >= 0) {
            lightest = std::min(lightest, load);
            heaviest = std::max(heaviest, load);
        }
    }
    for (int t = 0; t < n_tiles; t++)
        if (seen[t] != 1) return "a tile on no chain";
    if (g.per_wave && heaviest > 0 && heaviest - lightest > longest) return "a chain heavier than the lightest by more than the longest utterance";
    return "";
}

static std::vector<int64_t> list_of(const std::string &s) {
    std::vector<int64_t> v;
    if (s == "-") return v;
    std::stringstream ss(s);
    for (std::string t; std::getline(ss, t, ',');) v.push_back(std::stoll(t));
    return v;
}

static void print_report(const char *kind, const std::string &name, const Words &v) {  // (x86-64: an int64 in memory is its little-endian form)
    std::printf("%s %s %zu %s\n", kind, name.c_str(), v.size(), sha256(reinterpret_cast<const unsigned char *>(v.data()), v.size() * sizeof(int64_t)).c_str());
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string t; std::getline(ss, t, '\t');) f.push_back(t);
        if (f.size() < 5) return 2;
        const std::string kind = f[0], name = f[1];
        const int n_cu = std::stoi(f[2]);
        const std::vector<int64_t> lengths = list_of(f[3]), aux = list_of(f[4]);
        Design d(Opts::from_args(std::vector<std::string>(f.begin() + 5, f.end())));
        const Spread sp = spread_small_fft(d);
        std::string text;
        if (create_check(d, text) != CTU_OK) {
            std::fprintf(stderr, "%s: not an engine configuration: %s\n", name.c_str(), text.c_str());
            return 2;
        }
        const PlanGeom g = plan_geom(d, d.rows_in ? EngineTables() : build_engine_tables(d), sp, n_cu);  // as ctu_engine_create fills it
        HostPlan p;
        const int code = build_host_plan(g, lengths.data(), (int32_t)lengths.size(), p, text);
        n++;
        if (code != CTU_OK) {
            if (p.n_utt || !p.tiles.empty() || !p.sample_off.empty()) std::fprintf(stderr, "%s: a refused batch left a plan behind\n", name.c_str());
            std::printf("R %s %d %s\n", name.c_str(), code, hex(text).c_str());
            continue;
        }
        if (!g.rows_in)
            if (const std::string why = chains_breach(g, p); !why.empty()) std::fprintf(stderr, "%s: %s\n", name.c_str(), why.c_str());
        if (kind == "P") print_report("P", name, plan_report(p));
        else if (kind == "G") {
            const int order = (int)aux.at(0);
            const std::vector<int32_t> hidx(aux.begin() + 1, aux.end());
            if (hidx.size() != (size_t)p.n_utt) return 2;
            Words v;
            put(v, plan_ring_src(p, order, hidx.data()));
            for (int i = 0; i < p.n_utt; i++) {
                int32_t hi = hidx[i], hs = 0;
                vad_ring_step(order, p.frames[i], &hi, &hs);
                std::vector<int32_t> src((size_t)std::max<int64_t>(p.frames[i], 1), 0);
                const int64_t rows = vad_ring_rows(order, p.frames[i], hidx[i], src.data());
                v.insert(v.end(), {hi, hs, rows});
                v.insert(v.end(), src.begin(), src.begin() + rows);
            }
            print_report("G", name, v);
        } else if (kind == "S") {
            Words v;
            put(v, plan_part_first(p, (int)aux.at(0)));
            print_report("S", name, v);
        } else
            return 2;
    }
    std::printf("plan_check ok: %d cases\n", n);
    return 0;
}
