// Pipe mode of bin/ctucopy (-online_in / -online_out; the reference: rawIN::new_file on stdin, src/io/in.cc:268, and the writers' stream
// branches, src/io/out.cc:115-137,478): one stream of one stream set (include/ctu_engine.h: ctu_streams_*), fed as the bytes arrive.
//   pipe_take     how many of the samples that wait go into the next push: up to the one that completes the last frame whose index is
//                 7 (mod 8), so that every push ends a multiple of eight frames into the file - the condition under which the stream's
//                 rows and samples are those of the offline run bit for bit; at the end of input, all of them
//   PipeDecoder   bytes in, in reads that end anywhere - inside the WAVE header, in the middle of a sample -, whole elements out as they
//                 were read: G.711 codes, 16-bit samples in the input's byte order.  What they are worth is the stream set's to say
//                 (ctu_streams_push_wire_host with the decoder's layout) - or, for a caller that wants samples, wire_expand's
//   PipeOut       stdout (no HTK header: out.cc:115-137; raw: the samples alone) or -o's file, whose header is patched at close
//   run_pipe      read, accumulate, take, push, write and flush, until the input ends; then the stream's finish
// Host only.  pipe_take and PipeDecoder call nothing of the engine but the pure ctu_streams_step (and csrc/wire_layout.h, a header).
#pragma once
#include <cerrno>
#include <csignal>
#include <unistd.h>

#include "files.h"

// Samples of `buffered` (those read and not yet pushed, behind `pushed` samples of the file) that the next push takes.
inline int64_t pipe_take(int32_t window, int32_t wshift, int64_t pushed, int64_t buffered, bool eof) {
    if (eof) return buffered;
    const int64_t frames = ctu_streams_step(window, wshift, pushed + buffered, nullptr), whole = frames - frames % 8;
    if (whole <= 0) return 0;
    // frame t ends with sample t * wshift + window - 1: `whole` frames are complete after (whole - 1) * wshift + window samples
    return std::max<int64_t>((whole - 1) * (int64_t)wshift + window - pushed, 0);
}

// -format_in raw (either -endian_in) | alaw | mulaw | wave from a byte stream.  The WAVE header is the canonical 44 bytes, checked by the
// rules of files.h:wave_samples once they are all in; its data size bounds the samples taken, as it does for a file.
struct PipeDecoder {
    const ctu::Opts &o;
    const bool g711, alaw, wave, swap;
    uint8_t header[44];
    size_t header_have = 0;
    int64_t wave_left = 0;  // samples the data chunk still holds
    int half = -1;          // the first byte of a sample whose second has not arrived
    explicit PipeDecoder(const ctu::Opts &opts)
        : o(opts), g711(opts.format_in == "alaw" || opts.format_in == "mulaw"), alaw(opts.format_in == "alaw"), wave(opts.format_in == "wave"),
          swap(opts.swap_in && !wave) {
        if (o.format_in != "raw" && !g711 && !wave) throw Fatal("IN: Unknown input file format!");
    }
    // what an element of the accumulated bytes is: a code, or a 16-bit sample in the input's byte order
    ctu_wire_layout layout() const { return {g711 ? (alaw ? CTU_WIRE_ALAW : CTU_WIRE_MULAW) : swap ? CTU_WIRE_S16_SWAPPED : CTU_WIRE_S16, 1}; }
    size_t elem_bytes() const { return g711 ? 1 : 2; }
    // the whole elements of a read, appended to `out` byte for byte
    void feed_wire(const uint8_t *p, size_t n, std::vector<uint8_t> &out) {
        if (wave && header_have < 44) {
            const size_t k = std::min(n, 44 - header_have);
            std::memcpy(header + header_have, p, k);
            header_have += k;
            p += k;
            n -= k;
            if (header_have < 44) return;
            wave_left = wave_header_data_bytes(o, header) / 2;
        }
        if (n == 0) return;
        if (g711) {
            out.insert(out.end(), p, p + n);
            return;
        }
        size_t at = 0;
        if (half >= 0) {  // the byte kept from the read before, and the one that completes its sample
            const uint8_t first = (uint8_t)half;
            half = -1;
            at = 1;
            if (take_sample()) out.insert(out.end(), {first, p[0]});
        }
        size_t whole = (n - at) / 2;
        if (wave) {
            const size_t kept = (size_t)std::min<int64_t>((int64_t)whole, wave_left);
            wave_left -= (int64_t)kept;
            out.insert(out.end(), p + at, p + at + 2 * kept);
        } else out.insert(out.end(), p + at, p + at + 2 * whole);
        at += 2 * whole;
        if (at < n) half = p[at];
    }
    // ... and as samples, for a caller that has no stream set to expand them
    void feed(const uint8_t *p, size_t n, std::vector<int16_t> &out) {
        std::vector<uint8_t> raw;
        feed_wire(p, n, raw);
        const ctu_wire_layout w = layout();
        const size_t have = out.size(), more = raw.size() / elem_bytes();
        out.resize(have + more);
        wire_expand(&w, raw.data(), 0, (int64_t)more, out.data() + have);
    }
    // (a sample past the WAVE header's data size is dropped, as the file reader stops there)
    bool take_sample() {
        if (!wave) return true;
        if (wave_left <= 0) return false;
        wave_left--;
        return true;
    }
    // the end of input: a trailing half sample is dropped, as the file reader's n / 2 drops it
    void end() const {
        if (wave && header_have < 44) throw Fatal("IN: No RIFF header in file!");
    }
};

// Where a pipe's rows or samples go.  The stream or the file is opened with the first write or at close, whichever comes first: a run that
// fails ahead of its first row leaves what file mode leaves, nothing.
struct PipeOut {
    const ctu::Opts &o;
    const ctu_dims d;
    const bool to_stdout, signal, wave;
    FILE *f = nullptr;
    int64_t count = 0;  // rows, or samples
    PipeOut(const ctu::Opts &opts, const ctu_dims &dims)
        : o(opts), d(dims), to_stdout(opts.pipe_out), signal(opts.format_out == "raw" || opts.format_out == "wave"), wave(opts.format_out == "wave") {}
    PipeOut(const PipeOut &) = delete;
    ~PipeOut() {
        if (f && !to_stdout) std::fclose(f);
    }
    void open() {
        if (f) return;
        if (to_stdout) {
            f = stdout;
            return;
        }
        f = std::fopen(o.out.c_str(), "wb");
        if (!f) throw Fatal(wave ? "OUT: Cannot open data file!" : signal ? "OUT: Cannot open output stream!" : "OUT: Cannot create output file!");
        put_header();
    }
    void put_header() {
        const std::vector<uint8_t> h = wave ? wave_header((size_t)count, o.fs) : signal ? std::vector<uint8_t>() : htk_header(count, d);
        if (!h.empty() && std::fwrite(h.data(), 1, h.size(), f) != h.size()) throw Fatal("OUT: Error in stream writing!");
    }
    void rows(const float *r, int64_t n) {
        open();
        if (!put_rows(f, r, (size_t)n * d.row_floats, d.swap_out != 0) || std::fflush(f) != 0) throw Fatal("OUT: Error in stream writing!");
        count += n;
    }
    void samples(const int16_t *x, int64_t n) {
        open();
        if (!put_samples(f, x, (size_t)n, !wave && d.swap_out != 0) || std::fflush(f) != 0) throw Fatal("OUT: Error in stream writing!");
        count += n;
    }
    // the frame count of the HTK header, the sizes of the WAVE header (waveOUT::close, src/io/out.cc:548-564)
    void close() {
        open();
        if (!to_stdout && (wave || !signal)) {
            if (std::fseek(f, 0, SEEK_SET) != 0) throw Fatal("OUT: Error in stream writing!");
            put_header();
        }
        if (std::fflush(f) != 0) throw Fatal("OUT: Error in stream writing!");
        if (!to_stdout) {
            FILE *g = f;
            f = nullptr;
            if (std::fclose(g) != 0) throw Fatal("OUT: Error in stream writing!");
        }
    }
};

struct PipeSetFree {
    void operator()(ctu_streams *s) const { ctu_streams_destroy(s); }
};
struct PipeHostFree {
    void operator()(void *p) const { ctu_host_free(p); }
};

struct PipeJob {
    ctu_engine *eng = nullptr;
    uint32_t flags = 0;        // of ctu_streams_flags_for
    int32_t halo = 0;
    size_t read_bytes = 1 << 20;  // --pipe-read-bytes
    bool drop = false;         // -vad_apply_mode drop, done here: the set runs with `none`, a row whose decision is '0' is not written
    std::string vad_path;      // -vad_out with -vad_out_mode other than none
    int fd_in = 0;
};

// Returns the frames written (for the verbose line).  Throws Fatal with the text file mode has for the same bytes.
inline int64_t run_pipe(const PipeJob &job, const ctu::Opts &o, const ctu_dims &d) {
    ctu_engine *eng = job.eng;
    const bool signal = d.signal_out != 0, with_vad = (job.flags & CTU_STREAMS_VAD_STATE) != 0;
    PipeDecoder dec(o);
    std::signal(SIGPIPE, SIG_IGN);  // a reader that went away is a failed write, with the writer's message
    // a read brings at most read_samples, and fewer than 8 * wshift + window samples wait from the reads before it (pipe_take)
    const int64_t read_samples = (int64_t)(job.read_bytes / (dec.g711 ? 1 : 2)) + 1;
    const int64_t max_push = read_samples + 8 * (int64_t)d.wshift + d.window;
    // rows: the frames such a push completes at most, the wmax + 1 <= halo + 1 rows before them it may release, what a finish delivers
    const int64_t row_cap = ctu_streams_step(d.window, d.wshift, max_push + d.window, nullptr) + job.halo + 2;
    const int64_t sig_cap = ctu_streams_signal_step(d.window, d.wshift, max_push + d.window, nullptr) + d.window;
    ctu_streams *raw_set = nullptr;
    if (ctu_streams_create_ex(eng, 1, max_push, job.flags, &raw_set) != CTU_OK) throw Fatal(ctu_last_error(eng));
    std::unique_ptr<ctu_streams, PipeSetFree> set(raw_set);
    const size_t out_bytes = signal ? (size_t)sig_cap * sizeof(int16_t) : (size_t)row_cap * d.row_floats * sizeof(float);
    std::unique_ptr<void, PipeHostFree> out_buf(ctu_host_alloc(out_bytes));
    if (!out_buf) throw Fatal("ENGINE: page-locked memory for the rows of a pipe");
    float *h_rows = static_cast<float *>(out_buf.get());
    int16_t *h_sig = static_cast<int16_t *>(out_buf.get());
    std::vector<uint8_t> h_vad(with_vad ? (size_t)row_cap : 0);

    PipeOut out(o, d);
    File vad_file;
    // what a push or the finish delivered: to the writer, the decisions to -vad_out's file as they arrive
    auto deliver = [&](int64_t n) {
        if (n == 0) return;
        if (signal) return out.samples(h_sig, n);
        if (with_vad && !job.vad_path.empty()) {  // one ASCII '0' / '1' per frame (src/vad/vad.h:67-70)
            if (!vad_file) vad_file.reset(std::fopen(job.vad_path.c_str(), "wb"));
            if (!vad_file) throw Fatal("FileWriter: cannot open file!");
            if (std::fwrite(h_vad.data(), 1, (size_t)n, vad_file.get()) != (size_t)n || std::fflush(vad_file.get()) != 0) throw Fatal("OUT: Error in stream writing!");
        }
        if (!job.drop) return out.rows(h_rows, n);
        int64_t kept = 0;  // compacted in place: a row and its decision leave the stream together
        for (int64_t i = 0; i < n; i++)
            if (h_vad[(size_t)i] == '1') {
                if (kept != i) std::memmove(h_rows + kept * d.row_floats, h_rows + i * d.row_floats, (size_t)d.row_floats * sizeof(float));
                kept++;
            }
        if (kept) out.rows(h_rows, kept);
    };

    std::vector<uint8_t> bytes(job.read_bytes);
    std::vector<uint8_t> pend;  // whole elements read and not yet pushed, as they were read
    const ctu_wire_layout wire = dec.layout();
    const size_t unit = dec.elem_bytes();
    const int32_t id = 0;
    const int64_t from = 0;
    int64_t pushed = 0;
    for (bool eof = false; !eof;) {
        const ssize_t got = ::read(job.fd_in, bytes.data(), bytes.size());
        if (got < 0 && errno == EINTR) continue;
        if (got < 0) throw Fatal("IN: Cannot read data file!");
        eof = got == 0;
        if (eof) dec.end();
        else dec.feed_wire(bytes.data(), (size_t)got, pend);
        const int64_t waiting = (int64_t)(pend.size() / unit);
        if (eof && ctu_num_frames(eng, pushed + waiting) < 0) throw Fatal("IO: Signal shorter than one frame!");
        const int64_t take = pipe_take(d.window, d.wshift, pushed, waiting, eof);
        if (take == 0) continue;
        int64_t cnt = 0;  // the elements go up as read: the set expands codes and swaps bytes where it stitches them in
        const int rc = signal ? ctu_streams_push_signal_wire_host(set.get(), 1, &id, pend.data(), &from, &take, &wire, h_sig, sig_cap, &cnt)
                              : ctu_streams_push_wire_host(set.get(), 1, &id, pend.data(), &from, &take, &wire, h_rows, row_cap, &cnt,
                                                           with_vad ? h_vad.data() : nullptr);
        if (rc != CTU_OK) throw Fatal(ctu_last_error(eng));
        pend.erase(pend.begin(), pend.begin() + take * (int64_t)unit);
        pushed += take;
        deliver(cnt);
    }
    int64_t cnt = 0;
    const int rc = signal ? ctu_streams_finish_signal_host(set.get(), id, h_sig, sig_cap, &cnt)
                          : ctu_streams_finish_vad_host(set.get(), id, h_rows, row_cap, &cnt, with_vad ? h_vad.data() : nullptr);
    if (rc != CTU_OK) throw Fatal(ctu_last_error(eng));  // (a chain on too few frames: the offline plan's words)
    deliver(cnt);
    if (signal && ctu_streams_step(d.window, d.wshift, pushed, nullptr) == 0) {
        // window - wshift .. window - 1 samples: no frame, and the writer's close() still puts out its (all-zero) cache of window - wshift
        // samples (src/io/out.cc:487-491), as the offline run does; a stream's finish has nothing for a file without a frame
        std::fill(h_sig, h_sig + (d.window - d.wshift), (int16_t)0);
        deliver(d.window - d.wshift);
    }
    // VAD::new_file opens the file's VAD output whatever the file writes (a file of no more than (vad_filter_order - 1) / 2 frames: nothing)
    if (with_vad && !job.vad_path.empty() && !vad_file) write_file(job.vad_path, std::vector<uint8_t>(), "FileWriter: cannot open file!");
    out.close();
    return signal ? ctu_streams_step(d.window, d.wshift, pushed, nullptr) : out.count;
}
