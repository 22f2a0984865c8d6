// The host-only parts of offline wire input against brute force (tests/test_wire_offline_cpu.py builds and runs this under Address +
// UndefinedBehavior sanitizers; no engine library, no device):
//   list expansion and target naming             ctucopy_amd/host/wire_files.h: expand_channels, channel_target
//   the CLI's wire arena layout                   wire_arena_layout, and the element offsets main.cc derives from it
//   the covering range per part                   ctucopy_amd/csrc/wire_plan.h: wire_part_range
//   the bound check that precedes a launch        wire_unpack_fault
//   the pieces wire_unpack_kernel is dealt by     wire_pieces
// over small random lists: empty files, one-block files, N = 1, 2, 3, 8.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "wire_files.h"
#include "wire_plan.h"

static int failures = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                                \
        }                                                              \
    } while (0)

struct Item {
    std::string fin, fout, spk, fvad;
    int chan = 0;
};

static void check_targets() {
    CHECK(channel_target("a/b.htk", 1) == "a/b_1.htk");
    CHECK(channel_target("a/b.htk", 2) == "a/b_2.htk");
    CHECK(channel_target("b", 3) == "b_3");
    CHECK(channel_target("a.d/b", 1) == "a.d/b_1");
    CHECK(channel_target("a.d/b.c.raw", 12) == "a.d/b.c_12.raw");
    CHECK(channel_target("/x/y.", 1) == "/x/y_1.");
}

static void check_expansion(std::mt19937 &rng) {
    for (int n : {1, 2, 3, 8})
        for (int trial = 0; trial < 20; trial++) {
            std::vector<Item> items(rng() % 6);
            for (size_t i = 0; i < items.size(); i++) {
                items[i].fin = "in" + std::to_string(i) + ".raw";
                items[i].fout = (rng() % 2 ? "d.x/out" : "out") + std::to_string(i) + (rng() % 2 ? ".htk" : "");
                if (rng() % 2) items[i].spk = "s" + std::to_string(rng() % 3);
                if (rng() % 2) items[i].fvad = "v" + std::to_string(i) + ".vad";
            }
            const std::vector<Item> out = expand_channels(items, n);
            CHECK(out.size() == items.size() * (size_t)n);
            std::set<std::string> targets;
            for (size_t i = 0; i < items.size(); i++)      // brute force: file-major, channel-minor
                for (int c = 0; c < n; c++) {
                    const Item &o = out[i * n + c];
                    CHECK(o.fin == items[i].fin && o.spk == items[i].spk);
                    if (n == 1) {
                        CHECK(o.fout == items[i].fout && o.fvad == items[i].fvad && o.chan == 0);
                        continue;
                    }
                    CHECK(o.chan == c);
                    const std::string &f = items[i].fout;
                    const size_t dot = f.rfind('.'), slash = f.rfind('/');
                    const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
                    const std::string tag = "_" + std::to_string(c + 1);
                    CHECK(o.fout == (ext ? f.substr(0, dot) + tag + f.substr(dot) : f + tag));
                    CHECK(items[i].fvad.empty() ? o.fvad.empty() : o.fvad == "v" + std::to_string(i) + tag + ".vad");
                    CHECK(targets.insert(o.fout).second);
                }
        }
}

// the arena of a shard as main.cc lays it out, and every sample of every channel found where the layout says, once
static void check_arena(std::mt19937 &rng) {
    for (int n : {1, 2, 3, 8})
        for (int unit : {1, 2})
            for (int trial = 0; trial < 20; trial++) {
                const size_t files = rng() % 5;
                std::vector<int64_t> samples(files), file_bytes, byte_off;
                for (size_t f = 0; f < files; f++) {
                    const int kind = rng() % 4;
                    samples[f] = kind == 0 ? 0 : kind == 1 ? 1 : 1 + rng() % 40;  // empty files, one-block files, others
                    file_bytes.push_back(samples[f] * n * unit);
                }
                const int64_t total = wire_arena_layout(file_bytes, byte_off);
                CHECK(byte_off.size() == files);
                std::vector<int> owner((size_t)total, -1);
                int64_t prev_end = 0;
                for (size_t f = 0; f < files; f++) {
                    CHECK(byte_off[f] % 16 == 0 && byte_off[f] >= prev_end && byte_off[f] - prev_end < 16);
                    prev_end = byte_off[f] + file_bytes[f];
                    CHECK(prev_end <= total);
                    for (int64_t b = 0; b < file_bytes[f]; b++) {
                        CHECK(owner[(size_t)(byte_off[f] + b)] == -1);
                        owner[(size_t)(byte_off[f] + b)] = (int)f;
                    }
                }
                CHECK(total % 16 == 0 && total - prev_end < 16);
                // utterance (f, c): elem_off = byte_off / unit + c, stride n - the elements of block k of the file, channel c
                std::vector<int64_t> ns, eo;
                for (size_t f = 0; f < files; f++)
                    for (int c = 0; c < n; c++) {
                        ns.push_back(samples[f]);
                        eo.push_back(byte_off[f] / unit + c);
                    }
                std::vector<char> seen((size_t)total, 0);
                for (size_t u = 0; u < ns.size(); u++)
                    for (int64_t k = 0; k < ns[u]; k++) {
                        const int64_t byte = (eo[u] + k * n) * unit;
                        CHECK(byte + unit <= total && owner[(size_t)byte] == (int)(u / n));
                        CHECK(byte == byte_off[u / n] + (k * n + (int64_t)(u % n)) * unit);
                        CHECK(!seen[(size_t)byte]);
                        seen[(size_t)byte] = 1;
                    }
                // the covering range of every part [u0, u1), against the lowest and highest element its utterances name
                const ctu_wire_layout w = {unit == 1 ? CTU_WIRE_ALAW : CTU_WIRE_S16_SWAPPED, n};
                CHECK(wire_unpack_fault(&w, total ? (const void *)seen.data() : nullptr, (int)ns.size(), ns.data(), eo.data()).empty());
                for (size_t u0 = 0; u0 <= ns.size(); u0++)
                    for (size_t u1 = u0; u1 <= ns.size(); u1++) {
                        int64_t lo = INT64_MAX, hi = -1;
                        for (size_t u = u0; u < u1; u++)
                            for (int64_t k = 0; k < ns[u]; k++) {
                                lo = std::min(lo, eo[u] + k * n);
                                hi = std::max(hi, eo[u] + k * n);
                            }
                        int64_t first = -5;
                        std::vector<int64_t> rel(u1 - u0 + 1, -9);
                        const int64_t extent = wire_part_range(&w, (int)u0, (int)u1, ns.data(), eo.data(), &first, rel.data());
                        CHECK(extent == (hi < 0 ? 0 : hi - lo + 1));
                        CHECK(first == (hi < 0 ? 0 : lo));
                        for (size_t u = u0; u < u1; u++) CHECK(rel[u - u0] == (ns[u] ? eo[u] - first : 0));
                        CHECK(rel[u1 - u0] == -9);
                    }
            }
}

// the bound check: a set of utterances is refused exactly when an element it names lies below element 0, or the bytes from the buffer's
// start to its end cannot be counted in int64_t, the layout is none, or there is nothing to read from
static void check_bounds(std::mt19937 &rng) {
    const int64_t big = INT64_MAX;
    const int64_t offs[] = {0, 1, 17, -1, -big, big, big - 1, big / 2, big / 2 - 1, big / 2 + 1, big - 100};
    const int64_t lens[] = {0, 1, 2, 3, 101, big, big / 2};
    const int strides[] = {1, 2, 3, 8, INT32_MAX};
    char byte[4] = {0};
    for (int fmt = CTU_WIRE_S16; fmt <= CTU_WIRE_MULAW; fmt++)
        for (int stride : strides)
            for (int trial = 0; trial < 400; trial++) {
                const int n_utt = 1 + rng() % 3;
                std::vector<int64_t> ns, eo;
                bool bad = false, any = false;
                for (int i = 0; i < n_utt; i++) {
                    ns.push_back(lens[rng() % 7]);
                    eo.push_back(offs[rng() % 11]);
                    if (ns[i] == 0) continue;  // not looked at
                    any = true;
                    const __int128 last = (__int128)eo[i] + (__int128)(ns[i] - 1) * stride, unit = fmt >= CTU_WIRE_ALAW ? 1 : 2;
                    if (eo[i] < 0 || last > big || (last + 1) * unit > big) bad = true;  // (the bytes up to and with the last element are counted in int64_t)
                }
                const ctu_wire_layout w = {fmt, stride};
                const std::string why = wire_unpack_fault(&w, byte, n_utt, ns.data(), eo.data());
                CHECK(why.empty() == !bad);
                if (!any) CHECK(wire_unpack_fault(&w, nullptr, n_utt, ns.data(), eo.data()).empty());
                else if (!bad) CHECK(wire_unpack_fault(&w, nullptr, n_utt, ns.data(), eo.data()) == "wire: null buffer");
            }
    const int64_t one[] = {5}, at[] = {0}, neg[] = {-1}, zero[] = {0};
    ctu_wire_layout w = {CTU_WIRE_S16, 1};
    CHECK(wire_unpack_fault(nullptr, byte, 1, one, at) == "wire: null layout");
    CHECK(wire_unpack_fault(&w, byte + 1, 1, one, at).find("2-byte aligned") != std::string::npos);
    CHECK(wire_unpack_fault(&w, byte, 1, one, neg).find("negative element offset") != std::string::npos);
    CHECK(wire_unpack_fault(&w, byte, 1, zero, neg).empty());
    CHECK(wire_unpack_fault(&w, byte, 1, one, nullptr).find("null element offsets") != std::string::npos);
    w.format = 4;
    CHECK(wire_unpack_fault(&w, byte, 1, one, at).find("unknown format") != std::string::npos);
    w = {CTU_WIRE_ALAW, 0};
    CHECK(wire_unpack_fault(&w, byte, 1, one, at).find("stride below 1") != std::string::npos);
    w = {CTU_WIRE_ALAW, 1};
    CHECK(wire_unpack_fault(&w, byte + 1, 1, one, at).empty());  // codes lie at any address
}

// the pieces: for every arena sample, the search a lane makes between piece_first[b] and piece_first[b + 1] finds the utterance a scan finds
static void check_pieces(std::mt19937 &rng) {
    for (int trial = 0; trial < 200; trial++) {
        const int n_utt = 1 + rng() % 12;
        std::vector<int64_t> ns(n_utt), off(n_utt + 1);
        int64_t so = 8;
        for (int i = 0; i < n_utt; i++) {
            const int kind = rng() % 5;
            ns[i] = kind == 0 ? 0 : kind == 1 ? 1 + rng() % 8 : kind == 2 ? 1 + rng() % 300 : kind == 3 ? 2000 + rng() % 100 : 4096 + rng() % 5000;
            off[i] = so;
            so += (ns[i] + 7) / 8 * 8;
        }
        off[n_utt] = so;
        const std::vector<int> first = wire_pieces(off.data(), n_utt);
        const int64_t pieces = (so + WIRE_PIECE - 1) / WIRE_PIECE;
        CHECK((int64_t)first.size() == pieces + 1);
        for (int64_t a = 0; a < pieces * WIRE_PIECE; a += 8) {
            const int64_t b = a / WIRE_PIECE;
            int lo = first[(size_t)b], hi = first[(size_t)b + 1];
            CHECK(lo >= 0 && lo <= hi && hi < n_utt);
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= a) lo = mid;
                else hi = mid - 1;
            }
            int want = -1;  // the utterance that holds sample a
            for (int i = 0; i < n_utt; i++)
                if (a >= off[i] && a < off[i] + ns[i]) want = i;
            const int64_t k0 = a - off[lo], left = ns[lo] - k0;
            if (want >= 0) CHECK(lo == want && k0 >= 0 && left > 0);
            else CHECK(k0 < 0 || left <= 0);
            if (k0 >= 0 && left > 0) CHECK(a + std::min<int64_t>(left, 8) <= off[n_utt]);  // a lane stores inside the arena
        }
    }
    CHECK(wire_pieces(nullptr, 0).empty());
}

static void check_formats() {
    CHECK(wire_format_of("raw", false, 0) == -1 && wire_format_of("raw", false, 1) == -1 && wire_format_of("wave", false, 1) == -1);
    CHECK(wire_format_of("raw", true, 0) == CTU_WIRE_S16_SWAPPED && wire_format_of("raw", true, 2) == CTU_WIRE_S16_SWAPPED);
    CHECK(wire_format_of("raw", false, 2) == CTU_WIRE_S16 && wire_format_of("wave", false, 2) == CTU_WIRE_S16 && wire_format_of("wave", true, 2) == CTU_WIRE_S16);
    CHECK(wire_format_of("alaw", false, 0) == CTU_WIRE_ALAW && wire_format_of("mulaw", true, 3) == CTU_WIRE_MULAW);
    CHECK(wire_format_of("htk", false, 0) == -1);
}

int main() {
    std::mt19937 rng(20240607);
    check_targets();
    check_expansion(rng);
    check_arena(rng);
    check_bounds(rng);
    check_pieces(rng);
    check_formats();
    if (failures) {
        std::printf("wire_files_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("wire_files_check ok\n");
    return 0;
}
