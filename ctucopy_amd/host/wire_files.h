// Wire input of file mode (main.cc): which files go to the engine as they lie, how a list of N-channel files becomes the list of its
// channels, and where the files of a shard lie in its wire arena.  No engine call and no file is touched here:
// tests/host/wire_files_check.cc pins every function against brute force.
//
//   channel_target       `out` of a list line -> the target of channel c: _<c> ahead of the last extension
//   expand_channels      every `in out` line -> N mono lines, channel 1 .. N in that order: file-major, channel-minor, which is the order of
//                        everything a list has an order for (the *ss noise seed, the -vad file= stream, the majority filter's ring, CMVN's
//                        speakers, -vad_out, ark / pfile containers)
//   wire_format_of       the ctu_wire_layout format of -format_in / -endian_in, or -1 where the file path has nothing to expand and
//                        stays on ctu_engine_run_host (little-endian mono raw, mono WAVE)
//   wire_arena_layout    the files of a shard back to back, each starting at a multiple of 16 bytes
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ctu_engine.h"

constexpr int64_t WIRE_FILE_ALIGN = 16;  // bytes: a file's first element is where the widest load of wire_unpack_kernel is aligned

// a/b.htk -> a/b_1.htk; no extension (or a dot in a directory name only): appended
inline std::string channel_target(const std::string &out, int c) {
    const size_t slash = out.find_last_of('/'), dot = out.find_last_of('.');
    const std::string tag = "_" + std::to_string(c);
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return out + tag;
    return out.substr(0, dot) + tag + out.substr(dot);
}

// ItemT: fin, fout, spk, fvad (strings; the targets fout and fvad are renamed where they are set), chan (0-based)
template <class ItemT>
std::vector<ItemT> expand_channels(const std::vector<ItemT> &items, int n) {
    if (n <= 1) return items;
    std::vector<ItemT> out;
    out.reserve(items.size() * (size_t)n);
    for (const ItemT &it : items)
        for (int c = 0; c < n; c++) {
            ItemT ch = it;
            if (!it.fout.empty()) ch.fout = channel_target(it.fout, c + 1);
            if (!it.fvad.empty()) ch.fvad = channel_target(it.fvad, c + 1);
            ch.chan = c;
            out.push_back(ch);
        }
    return out;
}

inline int wire_format_of(const std::string &format_in, bool swap_in, int channels) {
    if (format_in == "alaw") return CTU_WIRE_ALAW;
    if (format_in == "mulaw") return CTU_WIRE_MULAW;
    if (format_in == "raw" && swap_in) return CTU_WIRE_S16_SWAPPED;
    if ((format_in == "raw" || format_in == "wave") && channels > 1) return CTU_WIRE_S16;
    return -1;
}

// byte_off[i]: where file i of file_bytes[i] bytes starts; returns the arena's bytes
inline int64_t wire_arena_layout(const std::vector<int64_t> &file_bytes, std::vector<int64_t> &byte_off) {
    byte_off.resize(file_bytes.size());
    int64_t at = 0;
    for (size_t i = 0; i < file_bytes.size(); i++) {
        byte_off[i] = at;
        at += (file_bytes[i] + WIRE_FILE_ALIGN - 1) / WIRE_FILE_ALIGN * WIRE_FILE_ALIGN;
    }
    return at;
}
