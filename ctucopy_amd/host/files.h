// Files into bytes and back for bin/ctucopy (main.cc): the reference's input decoders and its feature and signal writers, as they were in
// main.cc.  No engine call is made here: ctu_dims is used as a plain struct.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#include <sys/stat.h>
#include "ctu_engine.h"
#include "g711.h"
#include "opts.h"

struct Fatal : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// ---------------------------------------------------------------- decoders
inline uint32_t rd32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

struct FileCloser {
    void operator()(FILE *f) const {
        if (f) std::fclose(f);
    }
};
typedef std::unique_ptr<FILE, FileCloser> File;

// canonical 44-byte WAVE header only, like src/io/in.cc:550-597: the checks on its 44 bytes, in the reference's order; returns the data chunk's bytes.
// channels: what --channels says (0: nothing - the file is mono, as in the reference)
inline uint32_t wave_header_data_bytes(const ctu::Opts &o, const uint8_t *b, int channels = 0) {
    if (std::memcmp(b, "RIFF", 4)) throw Fatal("IN: No RIFF header in file!");
    if (std::memcmp(b + 8, "WAVE", 4)) throw Fatal("IN: Not a WAVE file!");
    if (rd16(&b[20]) != 1) throw Fatal("IN: Not a PCM WAVE file!");
    if ((long)rd32(&b[24]) != o.fs) throw Fatal("IN: WAVE file reports different sampling rate than specified!");
    if (channels > 0 && rd16(&b[22]) != channels)
        throw Fatal("IN: Input WAVE file holds " + std::to_string(rd16(&b[22])) + " channels, --channels says " + std::to_string(channels));
    if (channels <= 0 && rd16(&b[22]) != 1) throw Fatal("IN: Input WAVE file is not mono!");
    if (rd16(&b[34]) != 16) throw Fatal("IN: Not 16 bits per sample!");
    return rd32(&b[40]);
}
// returns the number of samples the file holds - per channel: an incomplete [sample][channel] block at the end is dropped
inline size_t wave_samples(const ctu::Opts &o, FILE *f, size_t file_bytes, int channels = 0) {
    uint8_t b[44];
    if (file_bytes < 44 || std::fread(b, 1, 44, f) != 44) throw Fatal("IN: No RIFF header in file!");
    const size_t block = 2 * (size_t)std::max(channels, 1);
    return std::min<size_t>(wave_header_data_bytes(o, b, channels) / block, (file_bytes - 44) / block);
}

// HTK feature file (htkIN::new_file / get_frame, src/io/in.cc:629-709): the 12-byte header in the byte order -endian_in names, its
// sampSize / 4 the row width of this file; the frame count is what the file really holds - get_frame stops at the first row it
// cannot read whole, the header's nSamples is never looked at.  htkIN's vector has -nfeacoefs entries for the life of the
// process (in.cc:623-627) and get_frame writes sampSize / 4 of them: a wider file writes past it, a narrower one leaves entries
// of the file before - neither is reproduced.
inline int64_t probe_htk_rows(const ctu::Opts &o, const std::string &path) {
    File f(std::fopen(path.c_str(), "rb"));
    if (!f) throw Fatal("IN: Cannot open data file!");
    uint8_t h[12];
    if (std::fread(h, 1, 12, f.get()) != 12) throw Fatal("OUT: Error in stream writing!\n");  // (sic: the reader throws the writer's text, in.cc:644-647)
    const int width = (o.swap_in ? (h[8] << 8 | h[9]) : rd16(&h[8])) / 4;
    if (width != o.nfeacoefs)
        throw Fatal("IN: " + path + " holds vectors of " + std::to_string(width) + " values, -nfeacoefs says " + std::to_string(o.nfeacoefs) +
                    " (the reference keeps one vector of -nfeacoefs entries for every file, src/io/in.cc:623-627,694-701)");
    // the rows are read in a second pass, at the offsets this one lays out: a stream that can be read only once (a FIFO) cannot be taken
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) throw Fatal("IN: " + path + " is not a regular file (feature input is sized first and read afterwards)");
    const size_t bytes = (size_t)st.st_size - 12;  // (the 12 header bytes have just been read: the file has them)
    return (int64_t)(bytes / (4 * (size_t)width));
}

// the payload of `n` rows as it stands in the file, into the words arena (the engine swaps and places the words)
inline void read_htk_rows(const ctu::Opts &o, const std::string &path, uint32_t *dst, size_t n) {
    File f(std::fopen(path.c_str(), "rb"));
    if (!f) throw Fatal("IN: Cannot open data file!");
    const size_t words = n * (size_t)o.nfeacoefs;
    if (std::fseek(f.get(), 12, SEEK_SET) != 0 || std::fread(dst, 4, words, f.get()) != words) throw Fatal("IN: Cannot read data file!");
}

// number of samples `path` will decode to, without reading its data; with --channels N (0: not given) the samples of one of its N
// interleaved channels - a trailing incomplete block of N elements is dropped, as an odd byte of a mono raw file is
inline int64_t probe_samples(const ctu::Opts &o, const std::string &path, int channels = 0) {
    if (o.format_in == "htk") return probe_htk_rows(o, path);
    const bool wave = o.format_in == "wave";
    if (o.format_in != "raw" && o.format_in != "alaw" && o.format_in != "mulaw" && !wave) throw Fatal("IN: Unknown input file format!");
    const size_t block = (size_t)std::max(channels, 1) * (o.format_in == "raw" ? 2 : 1);  // bytes of one sample of every channel (raw, G.711)
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
        // not a plain file (or missing): let fopen decide, sizes by reading to the end
        File f(std::fopen(path.c_str(), "rb"));
        if (!f) throw Fatal(wave ? "IN: Cannot open file!" : "IN: Cannot open data file!");
        size_t n = 0, got;
        uint8_t tmp[1 << 16];
        while ((got = std::fread(tmp, 1, sizeof tmp, f.get())) > 0) n += got;
        if (wave) {
            std::rewind(f.get());
            return (int64_t)wave_samples(o, f.get(), n, channels);
        }
        return (int64_t)(n / block);
    }
    const size_t bytes = (size_t)st.st_size;
    if (wave) {
        File f(std::fopen(path.c_str(), "rb"));
        if (!f) throw Fatal("IN: Cannot open file!");
        return (int64_t)wave_samples(o, f.get(), bytes, channels);
    }
    return (int64_t)(bytes / block);
}

// `bytes` bytes of the data of `path` as they lie in the file (raw / a-law / mu-law from the file's start, WAVE behind its 44-byte
// header): the one reader of file mode.  What there is to expand in them - G.711 codes, the other byte order, interleaved channels - the
// engine expands (wire input, main.cc); little-endian mono PCM is the samples themselves
inline void read_wire_bytes(const ctu::Opts &o, const std::string &path, void *dst, size_t bytes) {
    const bool wave = o.format_in == "wave";
    File f(std::fopen(path.c_str(), "rb"));
    if (!f) throw Fatal(wave ? "IN: Cannot open file!" : "IN: Cannot open data file!");
    if (wave && std::fseek(f.get(), 44, SEEK_SET) != 0) throw Fatal("IN: No RIFF header in file!");
    if (std::fread(dst, 1, bytes, f.get()) != bytes) throw Fatal("IN: Cannot read data file!");
}

// `n` samples of the mono file `path` as int16_t in dst (src/io/in.cc:434-619), for whoever needs samples on the host: the bytes as
// above, then wire_expand - the host statement of the expansion (csrc/wire_layout.h) - where the format has something to expand.  In
// place: the codes go to the upper half of the samples' own bytes and are expanded from the front (code i sits at byte n + i >= 2 i + 1)
inline void decode_into(const ctu::Opts &o, const std::string &path, int16_t *dst, size_t n) {
    const bool g711 = o.format_in == "alaw" || o.format_in == "mulaw", wave = o.format_in == "wave";
    uint8_t *bytes = reinterpret_cast<uint8_t *>(dst);
    read_wire_bytes(o, path, g711 ? bytes + n : bytes, g711 ? n : 2 * n);
    if (g711) {  // (wire_expand reads element k ahead of writing sample k, k ascending: what the in-place expansion rests on)
        const ctu_wire_layout w = {o.format_in == "alaw" ? CTU_WIRE_ALAW : CTU_WIRE_MULAW, 1};
        wire_expand(&w, bytes + n, 0, (int64_t)n, dst);
    } else if (o.swap_in && !wave) {
        const ctu_wire_layout w = {CTU_WIRE_S16_SWAPPED, 1};
        wire_expand(&w, bytes, 0, (int64_t)n, dst);
    }
}

// ---------------------------------------------------------------- writers
inline void put32(std::vector<uint8_t> &v, uint32_t x, bool big) {
    for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (big ? 24 - 8 * i : 8 * i)));
}
inline void put16(std::vector<uint8_t> &v, uint16_t x, bool big) {
    for (int i = 0; i < 2; i++) v.push_back((uint8_t)(x >> (big ? 8 - 8 * i : 8 * i)));
}
inline void putf(std::vector<uint8_t> &v, float f, bool big) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    put32(v, x, big);
}

inline void write_file(const std::string &path, const std::vector<uint8_t> &bytes, const char *err) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw Fatal(err);
    if (!bytes.empty() && std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
        std::fclose(f);
        throw Fatal("OUT: Error in stream writing!");
    }
    std::fclose(f);
}

// What file mode and pipe mode (pipe.h) share of the writers: the bytes of a header and of rows / samples, as the reference's writers lay
// them out.  The rows come from the engine in writer order (c1..cN, c0[, E]: include/ctu_engine.h), so placing c0 and E is done; what is
// left is the byte order of -endian_out.
// HTK: nSamples, sampPeriod (100 ns), sampSize (bytes), parmKind (src/io/out.cc:115-160)
inline std::vector<uint8_t> htk_header(int64_t n, const ctu_dims &d) {
    std::vector<uint8_t> h;
    const bool big = d.swap_out;
    put32(h, (uint32_t)n, big);
    put32(h, d.htk_period, big);
    put16(h, (uint16_t)(4 * d.row_floats), big);
    put16(h, (uint16_t)d.htk_kind, big);
    return h;
}
// nf float32 values of rows (src/io/out.cc:161-213); false: the stream refused them
inline bool put_rows(FILE *f, const float *rows, size_t nf, bool big) {
    if (nf == 0) return true;
    if (!big) return std::fwrite(rows, 4, nf, f) == nf;  // rows are little-endian float32 as they stand
    std::vector<uint32_t> sw(nf);
    for (size_t i = 0; i < nf; i++) {
        uint32_t x;
        std::memcpy(&x, rows + i, 4);
        sw[i] = __builtin_bswap32(x);
    }
    return std::fwrite(sw.data(), 4, nf, f) == nf;
}
// rawOUT::write (src/io/out.cc:493-499): int16 samples, byte-swapped for -endian_out big
inline bool put_samples(FILE *f, const int16_t *x, size_t n, bool big) {
    if (n == 0) return true;
    if (!big) return std::fwrite(x, 2, n, f) == n;
    std::vector<uint16_t> sw(n);
    for (size_t i = 0; i < n; i++) sw[i] = __builtin_bswap16((uint16_t)x[i]);
    return std::fwrite(sw.data(), 2, n, f) == n;
}
// waveOUT (src/io/out.cc:517-564): canonical 44-byte RIFF header for n samples
inline std::vector<uint8_t> wave_header(size_t n, int fs) {
    std::vector<uint8_t> b;
    const uint32_t data = (uint32_t)(2 * n);
    for (char c : std::string("RIFF")) b.push_back((uint8_t)c);
    put32(b, data + 36, false);
    for (char c : std::string("WAVEfmt ")) b.push_back((uint8_t)c);
    put32(b, 16, false);
    put16(b, 1, false);
    put16(b, 1, false);
    put32(b, (uint32_t)fs, false);
    put32(b, (uint32_t)fs * 2, false);
    put16(b, 2, false);
    put16(b, 16, false);
    for (char c : std::string("data")) b.push_back((uint8_t)c);
    put32(b, data, false);
    return b;
}

// HTK: the header, then float32 rows (src/io/out.cc:115-213)
inline void write_htk(const std::string &path, const float *rows, int64_t n, const ctu_dims &d) {
    const std::vector<uint8_t> h = htk_header(n, d);
    File f(std::fopen(path.c_str(), "wb"));
    if (!f) throw Fatal("OUT: Cannot create output file!");
    if (std::fwrite(h.data(), 1, h.size(), f.get()) != h.size() || !put_rows(f.get(), rows, (size_t)n * d.row_floats, d.swap_out != 0))
        throw Fatal("OUT: Error in stream writing!");
}

// KALDI binary matrix archive + index (src/io/out.cc:648-781)
struct ArkWriter {
    FILE *ark = nullptr, *scp = nullptr;
    std::string arkname;
    explicit ArkWriter(const std::string &name) : arkname(name) {
        ark = std::fopen(name.c_str(), "wb");
        if (!ark) throw Fatal("OUT: Cannot create output ark file!");
        // "x.ark" -> "x.scp": text up to the first ".ark" component, as rename_path_ark_to_scp does
        std::string scpname, rest = name;
        bool found = false;
        std::stringstream ss(name);
        std::string tok;
        while (std::getline(ss, tok, '.')) {
            if (tok.empty()) continue;
            if (tok == "ark") {
                found = true;
                break;
            }
            scpname += tok + ".";
        }
        (void)found;
        scpname += "scp";
        scp = std::fopen(scpname.c_str(), "wt");
        if (!scp) throw Fatal("Cannot open output scp file for writing!");
    }
    void add(const std::string &key, const float *rows, int64_t n, int cols) {
        std::fprintf(ark, "%s %cBFM %c", key.c_str(), 0, 4);
        const long long idx = (long long)ftello(ark) - 6;  // offset of the \0 that starts the binary marker
        const int32_t r = (int32_t)n, c = cols;
        std::fwrite(&r, 4, 1, ark);
        std::fputc(4, ark);
        std::fwrite(&c, 4, 1, ark);
        std::fprintf(scp, "%s %s:%lld\n", key.c_str(), arkname.c_str(), idx);
        if (n) std::fwrite(rows, 4, (size_t)n * cols, ark);
    }
    ~ArkWriter() {
        if (ark) std::fclose(ark);
        if (scp) std::fclose(scp);
    }
};

// ICSI pfile: 32768-byte ASCII header, big-endian rows [sent, frame, features], sentence index table
// (src/io/pfile.cc:435-468,470-505,573-592).  The reference opens it with the internal vector width, not the
// written row width (src/io/out.cc:252); that is reproduced: nfea_pf floats per row, zero padded / truncated.
struct PfileWriter {
    std::string name;
    int nfea;
    std::vector<uint8_t> data;
    std::vector<uint32_t> sent_start{0};
    uint32_t nframes = 0;
    // -format_in htk: pfileOUT::save_frame has no branch for feature input (src/io/out.cc:280-303, unlike htkOUT and arkOUT), so
    // it moves entry 0 of every block of fea_ncepcoefs+1 behind the others although the file's c0 is already there: rot = that block size
    int rot = 0;
    PfileWriter(const std::string &n, int nf) : name(n), nfea(nf) {}
    void add(const float *rows, int64_t n, int cols) {
        const uint32_t sid = (uint32_t)sent_start.size() - 1;
        for (int64_t t = 0; t < n; t++) {
            put32(data, sid, true);
            put32(data, (uint32_t)t, true);
            for (int i = 0; i < nfea; i++) {
                int c = i;
                if (rot && i < cols / rot * rot) c = i / rot * rot + (i % rot + 1) % rot;
                putf(data, c < cols ? rows[t * cols + c] : 0.f, true);
            }
        }
        nframes += (uint32_t)n;
        sent_start.push_back(nframes);
    }
    void close() {
        const unsigned long long hsize = 32768, dsize = (unsigned long long)(nfea + 2) * nframes;
        std::string h;
        char line[256];
        auto addf = [&](const char *fmt, auto... a) {
            std::snprintf(line, sizeof line, fmt, a...);
            h += line;
        };
        addf("-pfile_header version %u size %llu\n", 0u, hsize);
        addf("-num_sentences %u\n", (unsigned)sent_start.size() - 1);
        addf("-num_frames %u\n", nframes);
        addf("-first_feature_column %u\n", 2u);
        addf("-num_features %u\n", (unsigned)nfea);
        addf("-first_label_column %u\n", (unsigned)(2 + nfea));
        addf("-num_labels %u\n", 0u);
        h += "-format dd" + std::string(nfea, 'f') + "\n";
        addf("-data size %llu offset %llu ndim %u nrow %u ncol %u\n", dsize, 0ull, 2u, nframes, (unsigned)(nfea + 2));
        addf("-sent_table_data size %llu offset %llu ndim %u\n", (unsigned long long)sent_start.size(), dsize, 1u);
        h += "-end\n";
        std::vector<uint8_t> b(h.begin(), h.end());
        b.resize(hsize, 0);
        b.insert(b.end(), data.begin(), data.end());
        for (uint32_t s : sent_start) put32(b, s, true);
        write_file(name, b, "OUT: Cannot create output file!");
    }
};

// rawOUT: the samples alone
inline void write_raw(const std::string &path, const int16_t *x, size_t n, bool big) {
    File f(std::fopen(path.c_str(), "wb"));
    if (!f) throw Fatal("OUT: Cannot open output stream!");
    if (!put_samples(f.get(), x, n, big)) throw Fatal("OUT: Error in stream writing!");
}

// waveOUT: the header with its sizes, samples in host order
inline void write_wave(const std::string &path, const int16_t *x, size_t n, int fs) {
    const std::vector<uint8_t> b = wave_header(n, fs);
    File f(std::fopen(path.c_str(), "wb"));
    if (!f) throw Fatal("OUT: Cannot open data file!");
    if (std::fwrite(b.data(), 1, b.size(), f.get()) != b.size() || !put_samples(f.get(), x, n, false)) throw Fatal("OUT: Error in stream writing!");
}
