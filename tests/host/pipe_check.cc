// Stand-alone check of the host side of bin/ctucopy's pipe mode (ctucopy_amd/host/pipe.h, and what it shares with file mode in files.h):
// no engine library, no GPU, no HIP.  tests/test_pipe_host_cpu.py builds it with opts.cc under Address+UB sanitizers and runs it: exit
// status 0, a final "pipe_check ok" and a silent stderr are the result.
//
// pipe.h calls one function of the engine library, the pure ctu_streams_step.  This program states it as include/ctu_engine.h documents it
// (the frame count of ctu_num_frames, 0 while the file has none) and checks pipe_take against a count that does not go through it: frame t
// is complete once sample t * wshift + window - 1 is in.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pipe.h"

extern "C" int64_t ctu_streams_step(int32_t window, int32_t wshift, int64_t total, int64_t *carry) {
    const int64_t pre = window - wshift, F = total < pre ? 0 : (total - pre) / wshift;
    if (carry) *carry = total - F * wshift;
    return F;
}

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// ---- pipe_take
static int64_t frames_by_counting(int window, int wshift, int64_t total) {
    int64_t f = 0;
    while (f * wshift + window <= total) f++;
    return f;
}
// the largest prefix of the file's first `total` samples, no shorter than `pushed`, that ends a multiple of eight frames (and at least
// eight) into the file with the sample that completes the last of them
static int64_t take_by_search(int window, int wshift, int64_t pushed, int64_t buffered, bool eof) {
    if (eof) return buffered;
    for (int64_t n = pushed + buffered; n > pushed; n--) {
        const int64_t f = frames_by_counting(window, wshift, n);
        if (f > 0 && f % 8 == 0 && frames_by_counting(window, wshift, n - 1) == f - 1) return n - pushed;
    }
    return 0;
}
static void check_take() {
    const int shapes[4][2] = {{400, 160}, {1103, 441}, {200, 200}, {160, 200}};
    for (auto &s : shapes) {
        const int w = s[0], h = s[1];
        std::vector<int64_t> totals = {0, 1, w - 1, w, w + 1};
        for (int k = 1; k <= 4; k++)
            for (int e = -1; e <= 1; e++) totals.push_back((int64_t)(8 * k - 1) * h + w + e);  // the sample that completes frame 8 k - 1, one before, one after
        for (int64_t total : totals)
            for (int eof = 0; eof < 2; eof++) {
                // from the start of the file, and behind every push an earlier call could have made
                std::vector<int64_t> starts = {0};
                for (int k = 1; (int64_t)(8 * k - 1) * h + w <= total; k++) starts.push_back((int64_t)(8 * k - 1) * h + w);
                for (int64_t pushed : starts) {
                    const int64_t got = pipe_take(w, h, pushed, total - pushed, eof != 0), want = take_by_search(w, h, pushed, total - pushed, eof != 0);
                    CHECK(got == want);
                    CHECK(got >= 0 && got <= total - pushed);
                    if (!eof && got > 0) CHECK(frames_by_counting(w, h, pushed + got) % 8 == 0);
                    if (!eof) CHECK(frames_by_counting(w, h, total) - frames_by_counting(w, h, pushed + got) < 8);  // fewer than eight frames wait
                }
            }
        // a file walked in reads of every small size: the pushes are the same multiples of eight frames, and the end takes the rest
        for (int step : {1, 7, 159, 1024, 5000}) {
            int64_t pushed = 0, buffered = 0;
            const int64_t N = (int64_t)37 * h + w + 13;
            for (int64_t at = 0; at < N;) {
                const int64_t n = std::min<int64_t>(step, N - at);
                at += n;
                buffered += n;
                const int64_t t = pipe_take(w, h, pushed, buffered, false);
                pushed += t;
                buffered -= t;
                CHECK(t == 0 || frames_by_counting(w, h, pushed) % 8 == 0);
            }
            CHECK(frames_by_counting(w, h, pushed) == 32);
            CHECK(pipe_take(w, h, pushed, buffered, true) == buffered && pushed + buffered == N);
        }
    }
}

// ---- the byte accumulator
static ctu::Opts opts_of(const std::string &line) {
    std::vector<std::string> args;
    size_t at = 0;
    while (at < line.size()) {
        const size_t sp = line.find(' ', at);
        args.push_back(line.substr(at, sp - at));
        if (sp == std::string::npos) break;
        at = sp + 1;
    }
    return ctu::Opts::from_args(args);
}
static std::vector<int16_t> decode_in_reads(const ctu::Opts &o, const std::vector<uint8_t> &bytes, size_t read) {
    PipeDecoder dec(o);
    std::vector<int16_t> out;
    for (size_t at = 0; at < bytes.size(); at += read) dec.feed(bytes.data() + at, std::min(read, bytes.size() - at), out);
    dec.end();
    return out;
}
static std::vector<uint8_t> noise_bytes(size_t n) {
    std::vector<uint8_t> b(n);
    uint32_t x = 12345;
    for (size_t i = 0; i < n; i++) {
        x = x * 1664525u + 1013904223u;
        b[i] = (uint8_t)(x >> 24);
    }
    return b;
}
static void check_decoder() {
    const std::string tail = " -format_out htk -preset mfcc -i a -o b";
    const std::vector<uint8_t> bytes = noise_bytes(10001);  // an odd count: the last byte is half a sample
    struct Case {
        const char *args;
        int kind;  // 0 little-endian, 1 big-endian, 2 a-law, 3 mu-law
    } cases[] = {{"-fs 16000 -format_in raw -endian_in little", 0}, {"-fs 16000 -format_in raw -endian_in big", 1},
                 {"-fs 8000 -format_in alaw", 2}, {"-fs 8000 -format_in mulaw", 3}};
    for (const Case &c : cases) {
        const ctu::Opts o = opts_of(c.args + tail);
        std::vector<int16_t> want;
        if (c.kind >= 2)
            for (uint8_t b : bytes) want.push_back(g711_to_linear(b, c.kind == 2));
        else
            for (size_t i = 0; i + 1 < bytes.size(); i += 2)
                want.push_back((int16_t)(c.kind == 0 ? (uint16_t)(bytes[i] | bytes[i + 1] << 8) : (uint16_t)(bytes[i] << 8 | bytes[i + 1])));
        CHECK(decode_in_reads(o, bytes, bytes.size()) == want);
        for (size_t read : {1, 2, 3, 7, 4097}) CHECK(decode_in_reads(o, bytes, read) == want);
    }
    bool threw = false;
    try {
        PipeDecoder dec(opts_of("-fs 16000 -format_in htk -format_out htk -preset mfcc -i a -o b"));
    } catch (const Fatal &e) {
        threw = std::string(e.what()) == "IN: Unknown input file format!";
    }
    CHECK(threw);
}

// ---- the wave header
static std::vector<uint8_t> wave_image(const std::vector<uint8_t> &payload, uint32_t data_bytes, int fs, int format, int channels, int bits) {
    std::vector<uint8_t> b;
    for (char c : std::string("RIFF")) b.push_back((uint8_t)c);
    put32(b, data_bytes + 36, false);
    for (char c : std::string("WAVEfmt ")) b.push_back((uint8_t)c);
    put32(b, 16, false);
    put16(b, (uint16_t)format, false);
    put16(b, (uint16_t)channels, false);
    put32(b, (uint32_t)fs, false);
    put32(b, (uint32_t)fs * 2, false);
    put16(b, 2, false);
    put16(b, (uint16_t)bits, false);
    for (char c : std::string("data")) b.push_back((uint8_t)c);
    put32(b, data_bytes, false);
    b.insert(b.end(), payload.begin(), payload.end());
    return b;
}
static std::string refusal(const ctu::Opts &o, const std::vector<uint8_t> &img, size_t read) {
    try {
        decode_in_reads(o, img, read);
    } catch (const Fatal &e) {
        return e.what();
    }
    return "";
}
static void check_wave() {
    const ctu::Opts o = opts_of("-fs 16000 -format_in wave -format_out htk -preset mfcc -i a -o b");
    const std::vector<uint8_t> payload = noise_bytes(2001);
    std::vector<int16_t> want;
    for (size_t i = 0; i + 1 < payload.size(); i += 2) want.push_back((int16_t)(uint16_t)(payload[i] | payload[i + 1] << 8));
    const std::vector<uint8_t> img = wave_image(payload, 2000, 16000, 1, 1, 16);
    for (size_t read : {1, 5, 43, 44, 45, 4097}) CHECK(decode_in_reads(o, img, read) == want);
    // the data chunk's size bounds the samples (files.h:wave_samples): 600 bytes are 300 samples, whatever follows
    const std::vector<uint8_t> shorter = wave_image(payload, 600, 16000, 1, 1, 16);
    for (size_t read : {1, 5, 43, 44, 45}) CHECK(decode_in_reads(o, shorter, read) == std::vector<int16_t>(want.begin(), want.begin() + 300));
    for (size_t read : {1, 5, 43, 44, 45}) {
        CHECK(refusal(o, wave_image(payload, 2000, 16000, 3, 1, 16), read) == "IN: Not a PCM WAVE file!");
        CHECK(refusal(o, wave_image(payload, 2000, 8000, 1, 1, 16), read) == "IN: WAVE file reports different sampling rate than specified!");
        CHECK(refusal(o, wave_image(payload, 2000, 16000, 1, 2, 16), read) == "IN: Input WAVE file is not mono!");
        CHECK(refusal(o, wave_image(payload, 2000, 16000, 1, 1, 8), read) == "IN: Not 16 bits per sample!");
        CHECK(refusal(o, std::vector<uint8_t>(img.begin(), img.begin() + 43), read) == "IN: No RIFF header in file!");
        CHECK(refusal(o, std::vector<uint8_t>(), read) == "IN: No RIFF header in file!");
        CHECK(refusal(o, payload, read) == "IN: No RIFF header in file!");
    }
}

// ---- the shared row serialiser against the file writer
static std::vector<uint8_t> slurp(const std::string &path) {
    std::vector<uint8_t> b;
    File f(std::fopen(path.c_str(), "rb"));
    if (!f) return b;
    uint8_t tmp[4096];
    size_t got;
    while ((got = std::fread(tmp, 1, sizeof tmp, f.get())) > 0) b.insert(b.end(), tmp, tmp + got);
    return b;
}
static void check_serialiser(const std::string &dir) {
    for (int big = 0; big < 2; big++) {
        ctu_dims d;
        std::memset(&d, 0, sizeof d);
        d.row_floats = 13; d.htk_kind = 8198; d.htk_period = 100000; d.swap_out = big;
        std::vector<float> rows(7 * 13);
        for (size_t i = 0; i < rows.size(); i++) rows[i] = 0.37f * (float)i - 11.5f;
        const std::string by_file = dir + "/by_file.htk", by_parts = dir + "/by_parts.bin";
        write_htk(by_file, rows.data(), 7, d);
        const std::vector<uint8_t> whole = slurp(by_file);
        CHECK(whole.size() == 12 + 4 * rows.size());
        {
            File f(std::fopen(by_parts.c_str(), "wb"));  // in two pieces, as two pushes deliver them
            CHECK(f && put_rows(f.get(), rows.data(), 3 * 13, big != 0) && put_rows(f.get(), rows.data() + 3 * 13, 4 * 13, big != 0));
        }
        std::vector<uint8_t> parts = htk_header(7, d);
        CHECK(parts.size() == 12);
        const std::vector<uint8_t> payload = slurp(by_parts);
        parts.insert(parts.end(), payload.begin(), payload.end());
        CHECK(parts == whole);
        // ... and PipeOut on a file: header first, count patched at close
        ctu::Opts o = opts_of(std::string("-fs 16000 -format_in raw -format_out htk -preset mfcc -endian_out ") + (big ? "big" : "little") + " -online_in -o " + dir + "/by_pipe.htk");
        {
            PipeOut out(o, d);
            out.rows(rows.data(), 3);
            out.rows(rows.data() + 3 * 13, 4);
            out.close();
        }
        CHECK(slurp(dir + "/by_pipe.htk") == whole);
        // samples: raw in either byte order, wave with its sizes
        std::vector<int16_t> x(501);
        for (size_t i = 0; i < x.size(); i++) x[i] = (int16_t)(i * 131 - 30000);
        write_raw(dir + "/by_file.raw", x.data(), x.size(), big != 0);
        write_wave(dir + "/by_file.wav", x.data(), x.size(), 16000);
        ctu_dims ds = d;
        ds.signal_out = 1;
        for (const char *fmt : {"raw", "wave"}) {
            o = opts_of(std::string("-fs 16000 -format_in raw -format_out ") + fmt + " -preset exten -endian_out " + (big ? "big" : "little") + " -online_in -o " + dir + "/by_pipe.sig");
            PipeOut out(o, ds);
            out.samples(x.data(), 200);
            out.samples(x.data() + 200, 301);
            out.close();
            CHECK(slurp(dir + "/by_pipe.sig") == slurp(dir + (std::string(fmt) == "raw" ? "/by_file.raw" : "/by_file.wav")));
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::printf("usage: pipe_check <scratch directory>\n");
        return 2;
    }
    check_take();
    check_decoder();
    check_wave();
    check_serialiser(argv[1]);
    if (failures) {
        std::printf("pipe_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("pipe_check ok\n");
    return 0;
}
