// ctucopy -- command-line front end of the MI355X feature engine.
// Keeps the reference's command line (src/io/opts.cc:644-846), `-S` list format (`fin fout [spk] [vadfile]`, src/io/batch.cc:349-356),
// input decoders and feature writers (files.h), so that it is a drop-in for batch feature extraction.  The per-frame chain itself runs
// on the GPU(s) behind include/ctu_engine.h; this file only moves bytes, with the plumbing of pipeline.h.
// real_main is the list of steps - parse_host_flags, read_items, pipe_stage, make_engines, cut_at_end_of_vad_stream, open_writers, cmvn_stat_path,
// run_pipeline, cmvn_pass -; what they share is in Run, handed on by reference.
// pipe_stage is the whole run of -online_in (pipe.h): one stream of a stream set on the first engine, fed from stdin as the bytes arrive.
// -i <file> -online_out is the list of one file, whose writer is stdout (write_rows_out, write_signal_files).
// --channels N: every file of the list holds N interleaved channels; expand_channels makes the list the one of its channels - N items per
// line, file-major, channel-minor, targets out_<c> - ahead of batching, and a file's items stay together in a batch and on a GPU.
// run_pipeline (the counterpart of BATCH::process, src/io/batch.cc:326-421) has three stages that overlap batch by batch:
//   read_batches  - size_batch sizes the next files; fill_batch shards them over the GPUs by length (LPT; no collective: every utterance is
//                   independent) and reads them straight into page-locked arenas with a pool of I/O threads: little-endian mono PCM as the
//                   arena of samples, everything there is something to expand in - a-law, mu-law, the other byte order, interleaved
//                   channels - as the files lie, back to back (wire_files.h), for the device to expand;
//   run_batch     - one thread per GPU: run_shard = plan + ctu_engine_run_host (ctu_engine_run_wire_host) on its shard;
//   write_batches - write_batch: the verbose lines, then write_signal_files (raw / WAVE), stash_for_cmvn, or write_feature_files (HTK / VAD
//                   files by the same pool straight from the page-locked rows, ark / pfile in list order).
// A Batch owns its page-locked buffers (PinBuf) and a Plan its ctu_plan: both are given back where their holder dies, on every path.
// Files before a failing one are written as far as their batch got through, then the reference's message and exit status -1 (src/main.cpp:54-60).
// cmvn_pass (over the rows stash_for_cmvn kept): speaker_table, shard_corpus, cmvn_moment twice, write_cmvn_stats, then cmvn_apply_and_write,
// with vad_on_normalised_rows per file where the VAD is on.
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <thread>
#include <unordered_map>

#include "files.h"
#include "pipe.h"
#include "pipeline.h"
#include "wire_files.h"

namespace {

struct Item {
    std::string fin, fout, spk, fvad;
    int chan = 0;  // --channels: the channel of fin this item is, 0-based (expand_channels)
};
struct Gpu {
    ctu_engine *eng = nullptr;
    ~Gpu() {
        if (eng) ctu_engine_destroy(eng);
    }
};
struct PlanFree {
    void operator()(ctu_plan *p) const { ctu_plan_destroy(p); }
};
typedef std::unique_ptr<ctu_plan, PlanFree> Plan;
Plan make_plan(ctu_engine *eng, const std::vector<int64_t> &ns) {
    ctu_plan *plan = nullptr;
    if (ctu_plan_create(eng, ns.data(), (int)ns.size(), &plan) != CTU_OK) throw Fatal(ctu_last_error(eng));
    return Plan(plan);
}
// one GPU's part of a batch
struct Shard {
    std::vector<size_t> idx;      // positions in the batch, list order
    std::vector<int64_t> ns, so;  // samples per utterance, arena offsets (ctu_arena_layout)
    std::vector<int64_t> eo;      // wire input: every utterance's first element in the arena, which then holds the files' bytes as they lie
    std::vector<int32_t> hidx;    // VAD: the majority filter's ring index every utterance starts with (the list is one process's)
    int64_t total_samples = 0, total_frames = 0;
    PinBuf arena, rows;           // int16 in (wire input: the files back to back, wire_arena_layout); float32 rows (or int16 samples with -format_out raw|wave) out
    std::vector<int64_t> ro, kept, nout;
    std::vector<uint8_t> vad;
};
struct Batch {
    size_t pos = 0, n = 0;                        // items [pos, pos + n)
    std::vector<Shard> sh;                        // one per GPU
    std::vector<std::pair<int, size_t>> where;    // item -> (gpu, position in its shard)
    std::exception_ptr err;                       // the reader failed on this batch: rethrown once the earlier ones are through
    std::pair<Shard &, size_t> slot(size_t i) { return {sh[where[i].first], where[i].second}; }  // item i: its shard, its place there
};
typedef Chan<std::unique_ptr<Batch>> BatchChan;

struct Run {
    std::vector<std::string> args;  // the command line without the host's own flags: for ctu::Opts and the engines
    int ngpu = 1;
    std::vector<int> gpu_map;  // --gpu-map a,b,...: device ordinal of every engine (default 0 .. N-1); one may repeat: several engines on one device
    int io_threads = 0;     // --io-threads N: file readers (default: the hardware threads, at most 16)
    int write_threads = 0;  // --write-threads N: file writers (default 1: creating files in one directory does not scale)
    int batch_mib = 256;    // --batch-mib M: PCM per batch
    int channels = 0;       // --channels N: every input file interleaves N channels, each a file of the list in its own right (0: not given, mono)
    int wire_format = -1;   // CTU_WIRE_*: the files go to the engine as they lie (ctu_engine_run_wire_host); -1: decoded samples (wire_format_of)
    size_t pipe_read_bytes = 1 << 20;  // --pipe-read-bytes N: -online_in reads stdin in reads of at most N bytes
    bool pipe_drop = false;  // -online_in with -vad_apply_mode drop: the engine runs with `none`, the stage drops the rows (pipe_stage)
    ctu::Opts o;
    ctu_dims d;
    std::vector<Item> items;
    std::vector<Gpu> gpus;
    PinPool pool{ctu_host_alloc, ctu_host_free};  // outlives every Batch and both threads: those are run_pipeline's
    bool signal_out = false, cmvn = false, cmvn_vad = false, vad_ring = false;
    std::unique_ptr<ArkWriter> ark;
    std::unique_ptr<PfileWriter> pf;
    std::vector<std::vector<float>> all_rows;  // -stat_cmvn / -apply_cmvn: the corpus waits for its statistics
    std::vector<int64_t> all_ns;
    std::vector<std::vector<uint8_t>> all_vads;
    double t_read = 0, t_engine = 0, t_write = 0;  // CTU_HOST_TIMING=1: seconds each stage was busy (not waiting for its neighbours)
};
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int env_threads(const char *name, int otherwise) {
    const char *ev = std::getenv(name);
    return ev ? std::max(1, std::atoi(ev)) : otherwise;
}
void parse_host_flags(Run &r, int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) r.ngpu = std::max(1, std::atoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--io-threads") && i + 1 < argc) r.io_threads = std::max(1, std::atoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--write-threads") && i + 1 < argc) r.write_threads = std::max(1, std::atoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--batch-mib") && i + 1 < argc) r.batch_mib = std::max(1, std::atoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--channels")) {
            char *end = nullptr;
            const long n = i + 1 < argc ? std::strtol(argv[++i], &end, 10) : 0;
            if (!end || end == argv[i] || *end || n < 1 || n > INT32_MAX) throw Fatal("ENGINE: --channels needs the number of interleaved channels of every input file, 1 or more");  // (a ctu_wire_layout's stride is an int32_t)
            r.channels = (int)n;
        }
        else if (!std::strcmp(argv[i], "--pipe-read-bytes") && i + 1 < argc) r.pipe_read_bytes = (size_t)std::min(std::max(1ll, std::atoll(argv[++i])), 1ll << 25);  // (a push holds at most 2^26 samples)
        else if (!std::strcmp(argv[i], "--gpu-map") && i + 1 < argc) {
            std::istringstream ms(argv[++i]);
            std::string tok;
            while (std::getline(ms, tok, ',')) r.gpu_map.push_back(std::atoi(tok.c_str()));
        }
        else r.args.emplace_back(argv[i]);
    }
    if (r.io_threads == 0) r.io_threads = env_threads("CTU_IO_THREADS", (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
    if (r.write_threads == 0) r.write_threads = env_threads("CTU_WRITE_THREADS", 1);
    if (!r.gpu_map.empty() && (int)r.gpu_map.size() != r.ngpu) throw Fatal("ENGINE: --gpu-map needs one device ordinal per engine of --gpus");
}
// the work list: -i / -o, or the -S list
std::vector<Item> read_items(const ctu::Opts &o) {
    if (o.pipe_in) return {};  // stdin is no list: pipe_stage
    if (!o.in.empty()) return {{o.in, o.out, "", o.vad_out}};  // (-online_out: no name, the writers take stdout)
    if (o.list.empty()) throw Fatal("BATCH: Nothing to do!");
    std::ifstream lf(o.list);
    if (!lf) throw Fatal("BATCH: Cannot open list file!");
    std::vector<Item> items;
    std::string line;
    while (std::getline(lf, line)) {
        std::istringstream ss(line);
        Item it;
        if (!(ss >> it.fin >> it.fout)) {
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            throw Fatal("BATCH: Bad list format!");
        }
        ss >> it.spk >> it.fvad;
        if (o.do_vad() && it.fvad.empty()) throw Fatal("BATCH: Bad list format!");
        // CMVN lists (src/io/batch.cc:358-367): "<in> <speaker>" when only statistics are wanted, "<in> <out> <speaker>" when they are applied
        if (o.apply_cmvn && it.spk.empty()) throw Fatal(" Bad list format for applying cmvn!");
        if (o.stat_cmvn && it.spk.empty()) it.spk = it.fout;
        items.push_back(it);
    }
    return items;
}
void make_engines(Run &r) {
    std::vector<const char *> cargs;
    for (auto &a : r.args) cargs.push_back(a.c_str());
    // CMVN together with the VAD (src/io/batch.cc:193-204,230-241): the statistics are taken over every frame (the passes that sum do not
    // call save_frame, so the VAD does not see them), the last pass normalises a vector and THEN hands it to save_frame - the VAD's ring,
    // its decision, the drop.  The engine therefore delivers every row (apply mode none) and cmvn_pass does the VAD's part on the
    // normalised rows: the ring's phase along the list, the rows a short file does not write, the dropped frames.
    if (r.cmvn_vad || r.pipe_drop) {  // (a pipe with -vad_apply_mode drop likewise: pipe_stage)
        cargs.push_back("-vad_apply_mode");
        cargs.push_back("none");
    }
    r.gpus = std::vector<Gpu>(r.ngpu);
    for (int g = 0; g < r.ngpu; g++)
        if (ctu_engine_create((int)cargs.size(), cargs.data(), r.gpu_map.empty() ? g : r.gpu_map[g], &r.gpus[g].eng) != CTU_OK) throw Fatal(ctu_create_error());
    ctu_engine_dims(r.gpus[0].eng, &r.d);
}
// -vad file=<f> with hwss / fwss / 2fwss: `char vad = fgetc(fvad); if (vad != EOF) ... else throw` (src/nr/nr.cc:297-302) - the reference
// runs out of decisions at some FRAME, after every file in front of that one has been written.  The engine takes a batch whole, so
// the list is cut in front of the file whose frames pass the end of the stream (or its first 0xFF byte, which the signed char
// compares equal to EOF) and the reference's message is returned, to be raised once the files before it are out.
std::string cut_at_end_of_vad_stream(Run &r) {
    std::ifstream vf(r.o.filevad, std::ios::binary);
    if (!vf) return "";
    std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(vf)), std::istreambuf_iterator<char>());
    int64_t usable = (int64_t)(std::find(bytes.begin(), bytes.end(), (unsigned char)0xFF) - bytes.begin()), used = 0;
    int64_t T = -1;
    for (size_t i = 0; i < r.items.size(); i++) {
        try {
            if (r.items[i].chan == 0) T = ctu_num_frames(r.gpus[0].eng, probe_samples(r.o, r.items[i].fin, r.channels));  // (a file is asked once: its channels are equally long)
        } catch (...) {
            break;  // the reader reports the unreadable file where the reference would
        }
        if (T < 0) break;
        if (used + T > usable) {
            r.items.resize(i);
            return "NR: Unexpected end of VAD file!";
        }
        used += T;
    }
    return "";
}
void open_writers(Run &r) {
    const ctu::Opts &o = r.o;
    if (o.format_out == "ark") r.ark.reset(new ArkWriter(o.arkfilename));
    if (o.format_out == "pfile") {
        // internal vector width: row width without E, plus c0 when it is switched off for the row (src/io/out.cc:252)
        int nfea_pf = r.d.row_floats - (o.fea_E ? 1 : 0);
        if ((o.fea_kind == "dctc" || o.fea_kind == "lpc") && !o.fea_c0) nfea_pf += 1;
        if (o.fea_kind == "lpa") nfea_pf += 1;
        r.pf.reset(new PfileWriter(o.pfilename, nfea_pf));
        if (o.format_in == "htk" && !o.fea_trap && (o.fea_kind == "dctc" || o.fea_kind == "lpc")) r.pf->rot = o.fea_ncepcoefs + 1;
    }
}
// ---- per-speaker CMVN (src/io/batch.cc:131-171,331-419).  -apply_cmvn <f>: the reference first tries to read <f>; its reader keeps "mean" as
// every speaker's name and only fea_ncepcoefs+1 values (src/io/in.cc:735-770), after which add_spk allocates fresh all-zero statistics for each
// real speaker - the run divides by zero.  That path is not reproduced.  When <f> does not exist the reference computes the statistics, writes
// them to <f> and applies them in a third pass; -stat_cmvn <f> alone computes and writes them and produces no feature files.
std::string cmvn_stat_path(const ctu::Opts &o) {
    if (!o.apply_cmvn) return o.fcmvn_stat_out;
    if (std::ifstream(o.fcmvn_stat_in).good())
        throw Fatal("ENGINE: applying an existing CMVN statistics file is not on the accelerated path (the reference's reader loses the speaker names and the statistics, src/io/in.cc:735-770)");
    std::printf("IN: Cannot open stat. cmvn file!\nIN: Stat. cmvn file is being created: %s\n", o.fcmvn_stat_in.c_str());
    return o.fcmvn_stat_in;
}
// At filter orders of 5 and more a file with no more frames than the filter's delay leaves the reference's historySize half drained (one
// flush_frame per unready file, src/vad/vad.h:156-175): the file behind it gets ready early and writes more rows and decisions than it
// has frames.  Not reproduced - and not passed over in silence.
Fatal half_drained(const Run &r, size_t short_file) {
    return Fatal("VAD: " + r.items[short_file].fin + " has no more frames than the majority filter delays (-vad_filter_order " + std::to_string(r.o.vad_filter_order) +
                 "): the reference's filter stays half drained for the files behind it (src/vad/vad.h:156-175), which is not reproduced");
}
struct ListCursor {
    size_t pos = 0;
    int32_t ring_hidx = 0, ring_hsize = 0;
    // sizes of the files probed so far (a group is probed ahead of the batch it fills: what the batch leaves is not probed again)
    std::vector<int64_t> probed;
    std::vector<std::exception_ptr> probe_err;
};
// sizes first (stat, WAVE headers), in groups, until the batch is full: the lengths of the batch's files, from c.pos on
std::vector<int64_t> size_batch(Run &r, ListCursor &c) {
    const size_t batch_samples = (size_t)r.batch_mib << 19;  // samples of PCM per batch (default 1 GiB)
    const size_t unit = r.d.rows_in ? 2 * (size_t)r.d.row_floats_in : 1;  // -format_in htk: a "sample" is a row of that many floats, batches stay sized in bytes
    const size_t nch = (size_t)std::max(r.channels, 1);  // the channels of a file stay in one batch: it ends between files only
    std::vector<int64_t> ns;
    size_t total = 0, end = c.pos;
    bool stop = false;
    auto room = [&] { return total < batch_samples || end == c.pos || (end - c.pos) % nch != 0; };
    while (!stop && end < r.items.size() && room()) {
        if (end >= c.probed.size()) {
            const size_t first = c.probed.size(), group = std::min<size_t>(r.items.size() - first, 1024);
            c.probed.resize(first + group);
            c.probe_err.resize(first + group);
            parallel_for(r.io_threads, group, [&](size_t i) {
                if (r.items[first + i].chan != 0) return;  // a file is asked once, with its first channel
                try {
                    c.probed[first + i] = probe_samples(r.o, r.items[first + i].fin, r.channels);
                    if (ctu_num_frames(r.gpus[0].eng, c.probed[first + i]) < 0) throw Fatal("IO: Signal shorter than one frame!");
                } catch (...) {
                    c.probe_err[first + i] = std::current_exception();
                }
            });
            for (size_t i = first; i < first + group; i++)  // its other channels are as long (their first may lie in the group before)
                if (r.items[i].chan != 0) {
                    c.probed[i] = c.probed[i - 1];
                    c.probe_err[i] = c.probe_err[i - 1];
                }
        }
        for (; end < c.probed.size() && room(); end++) {
            if (c.probe_err[end]) {  // a bad file ends the batch in front of it; it fails the batch it would start
                if (end == c.pos) std::rethrow_exception(c.probe_err[end]);
                stop = true;
                break;
            }
            ns.push_back(c.probed[end]);
            total += (size_t)c.probed[end] * unit;
        }
    }
    return ns;
}
// shards the files of lengths `ns` over the GPUs, takes the arenas and reads the files into them
void fill_batch(Run &r, ListCursor &c, Batch &b, const std::vector<int64_t> &ns) {
    const ctu_dims &d = r.d;
    const size_t n = b.n = ns.size();
    // longest-processing-time sharding over the GPUs by length; list order inside a shard.  What is dealt is a file: with --channels its
    // nch items, which follow each other and are equally long, go to one GPU
    const size_t nch = (size_t)std::max(r.channels, 1), files = n / nch;
    std::vector<size_t> order(files);
    for (size_t i = 0; i < files; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ns[x * nch] > ns[y * nch]; });
    b.sh.resize(r.ngpu);
    std::vector<size_t> load(r.ngpu, 0);
    for (size_t f : order) {
        const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        for (size_t c_ = 0; c_ < nch; c_++) b.sh[g].idx.push_back(f * nch + c_);
        load[g] += (size_t)ns[f * nch] * nch;
    }
    b.where.resize(n);
    std::vector<int32_t> hidx_of(n, 0);
    if (r.vad_ring)
        for (size_t i = 0; i < n; i++) {  // list order
            if (c.ring_hsize != 0) throw half_drained(r, b.pos + i - 1);
            hidx_of[i] = c.ring_hidx;
            ctu_vad_ring_step(r.o.vad_filter_order, std::max<int64_t>(ctu_num_frames(r.gpus[0].eng, ns[i]), 0), &c.ring_hidx, &c.ring_hsize);
        }
    for (int g = 0; g < r.ngpu; g++) {
        Shard &sh = b.sh[g];
        std::sort(sh.idx.begin(), sh.idx.end());
        for (size_t k = 0; k < sh.idx.size(); k++) {
            sh.ns.push_back(ns[sh.idx[k]]);
            if (r.vad_ring) sh.hidx.push_back(hidx_of[sh.idx[k]]);
            b.where[sh.idx[k]] = {g, k};
        }
        sh.so.resize(sh.ns.size() + 1);
        sh.total_samples = d.rows_in ? ctu_rows_arena_layout(sh.ns.data(), (int)sh.ns.size(), d.row_floats_in, sh.so.data()) : ctu_arena_layout(sh.ns.data(), (int)sh.ns.size(), sh.so.data());
        if (sh.idx.empty()) continue;
        if (r.wire_format >= 0) {  // the files as they lie, back to back: utterance k is channel `chan` of its file, nch elements from sample to sample
            const int64_t unit = r.wire_format == CTU_WIRE_ALAW || r.wire_format == CTU_WIRE_MULAW ? 1 : 2;
            std::vector<int64_t> file_bytes, byte_off;
            for (size_t k = 0; k < sh.idx.size(); k += nch) file_bytes.push_back(sh.ns[k] * (int64_t)nch * unit);
            sh.arena = r.pool.get((size_t)std::max<int64_t>(wire_arena_layout(file_bytes, byte_off), 1));
            for (size_t k = 0; k < sh.idx.size(); k++) sh.eo.push_back(byte_off[k / nch] / unit + r.items[b.pos + sh.idx[k]].chan);
            continue;
        }
        // the bytes between utterances are read under zero weights and need no particular value (include/ctu_engine.h)
        sh.arena = r.pool.get((size_t)sh.total_samples * (d.rows_in ? sizeof(uint32_t) : sizeof(int16_t)));
    }
    parallel_for(r.io_threads, n, [&](size_t i) {
        auto [sh, k] = b.slot(i);
        const Item &it = r.items[b.pos + i];
        if (d.rows_in) read_htk_rows(r.o, it.fin, static_cast<uint32_t *>(sh.arena.get()) + sh.so[k], (size_t)sh.ns[k]);
        else if (r.wire_format < 0) decode_into(r.o, it.fin, static_cast<int16_t *>(sh.arena.get()) + sh.so[k], (size_t)sh.ns[k]);
        else if (it.chan == 0) {  // a file is read once, where its first channel starts
            const size_t unit = r.wire_format == CTU_WIRE_ALAW || r.wire_format == CTU_WIRE_MULAW ? 1 : 2;
            read_wire_bytes(r.o, it.fin, static_cast<uint8_t *>(sh.arena.get()) + (size_t)sh.eo[k] * unit, (size_t)sh.ns[k] * nch * unit);
        }
    });
}
void read_batches(Run &r, BatchChan &to_engine, const std::atomic<bool> &giving_up) {
    ListCursor c;
    while (c.pos < r.items.size() && !giving_up) {
        std::unique_ptr<Batch> b(new Batch);
        b->pos = c.pos;
        const double t0 = now();
        try {
            fill_batch(r, c, *b, size_batch(r, c));
            c.pos += b->n;
            r.t_read += now() - t0;
        } catch (...) {
            b->sh.clear();  // the page-locked arenas already taken for this batch go back to the pool
            b->err = std::current_exception();
            to_engine.push(std::move(b));
            break;
        }
        if (!to_engine.push(std::move(b))) break;
    }
    to_engine.close();
}
// the engine's part of a shard: plan over its lengths, H2D + kernels + D2H from / to the page-locked buffers
void run_shard(Run &r, ctu_engine *eng, Shard &sh) {
    const ctu_dims &d = r.d;
    const Plan holder = make_plan(eng, sh.ns);
    ctu_plan *plan = holder.get();
    const size_t n = sh.ns.size();
    const int64_t *so = ctu_plan_sample_offsets(plan), *ro = ctu_plan_row_offsets(plan);
    if (ctu_plan_total_samples(plan) != sh.total_samples || !std::equal(sh.so.begin(), sh.so.end(), so))
        throw Fatal("ENGINE: internal: the plan's arena layout differs from ctu_arena_layout / ctu_rows_arena_layout");
    if (!sh.hidx.empty() && ctu_plan_set_vad_ring(plan, sh.hidx.data()) != CTU_OK) throw Fatal(ctu_last_error(eng));
    sh.total_frames = ctu_plan_total_frames(plan);
    sh.ro.assign(ro, ro + n + 1);
    sh.kept.assign(n, 0);
    const ctu_wire_layout wire = {r.wire_format, std::max(r.channels, 1)};  // (wire input: the files as they lie, an utterance per channel)
    if (r.signal_out) {  // -format_out raw|wave: samples at the utterances' own offsets (ctu_engine_run_signal_host)
        sh.rows = r.pool.get((size_t)sh.total_samples * sizeof(int16_t));
        const int64_t *no = ctu_plan_out_samples(plan);
        sh.nout.assign(no, no + n);
        const int rc = r.wire_format >= 0 ? ctu_engine_run_signal_wire_host(eng, plan, sh.arena.get(), sh.eo.data(), &wire, static_cast<int16_t *>(sh.rows.get()))
                                          : ctu_engine_run_signal_host(eng, plan, static_cast<const int16_t *>(sh.arena.get()), static_cast<int16_t *>(sh.rows.get()));
        if (rc != CTU_OK) throw Fatal(ctu_last_error(eng));
        return;
    }
    sh.rows = r.pool.get((size_t)sh.total_frames * d.row_floats * sizeof(float));
    sh.vad.assign(d.has_vad ? (size_t)sh.total_frames : 0, 0);
    // rows_per_utt < frames only with -vad_apply_mode drop (rows compacted in place by the library)
    if (d.rows_in) {  // -format_in htk: every row of the file comes out (no VAD on this path)
        for (size_t i = 0; i < n; i++) sh.kept[i] = ro[i + 1] - ro[i];
        if (ctu_engine_run_rows_host(eng, plan, sh.arena.get(), static_cast<float *>(sh.rows.get())) != CTU_OK) throw Fatal(ctu_last_error(eng));
        return;
    }
    uint8_t *vad = d.has_vad ? sh.vad.data() : nullptr;
    const int rc = r.wire_format >= 0 ? ctu_engine_run_wire_host(eng, plan, sh.arena.get(), sh.eo.data(), &wire, static_cast<float *>(sh.rows.get()), vad, sh.kept.data())
                                      : ctu_engine_run_host(eng, plan, static_cast<const int16_t *>(sh.arena.get()), static_cast<float *>(sh.rows.get()), vad, sh.kept.data());
    if (rc != CTU_OK) throw Fatal(ctu_last_error(eng));
}
void run_batch(Run &r, Batch &b) {
    per_gpu(r.ngpu, [&](int g) {
        if (!b.sh[g].idx.empty()) run_shard(r, r.gpus[g].eng, b.sh[g]);
    });
}
// -online_out: one file in, its bytes to stdout as the reference's writers put them on a stream - rows without the HTK header
// (src/io/out.cc:115-137), samples alone (out.cc:478)
void to_stdout(bool ok) {
    if (!ok || std::fflush(stdout) != 0) throw Fatal("OUT: Error in stream writing!");
}
void write_rows_out(const Run &r, const std::string &path, const float *rows, int64_t nr, const ctu_dims &dh) {
    if (r.o.pipe_out) to_stdout(put_rows(stdout, rows, (size_t)nr * dh.row_floats, dh.swap_out != 0));
    else write_htk(path, rows, nr, dh);
}
std::pair<const float *, int64_t> rows_of(const Run &r, Batch &b, size_t i) {
    auto [sh, k] = b.slot(i);
    return {static_cast<const float *>(sh.rows.get()) + sh.ro[k] * r.d.row_floats, sh.kept[k]};
}
// speech enhancement: samples instead of rows (src/io/batch.cc:62-65,223-227)
void write_signal_files(Run &r, Batch &b) {
    parallel_for(r.write_threads, b.n, [&](size_t i) {
        auto [sh, k] = b.slot(i);
        const int16_t *x = static_cast<const int16_t *>(sh.rows.get()) + sh.so[k];
        if (r.o.pipe_out) to_stdout(put_samples(stdout, x, (size_t)sh.nout[k], r.d.swap_out != 0));  // (raw: the parser refuses wave here)
        else if (r.o.format_out == "raw") write_raw(r.items[b.pos + i].fout, x, (size_t)sh.nout[k], r.d.swap_out != 0);
        else write_wave(r.items[b.pos + i].fout, x, (size_t)sh.nout[k], r.o.fs);
    });
}
// rows wait for the corpus statistics
void stash_for_cmvn(Run &r, Batch &b) {
    for (size_t i = 0; i < b.n; i++) {
        auto [rows, nr] = rows_of(r, b, i);
        auto [sh, k] = b.slot(i);
        if (r.cmvn_vad) {  // every frame's row counts for the statistics, also those of a file the VAD writes nothing for
            nr = sh.ro[k + 1] - sh.ro[k];
            r.all_vads[b.pos + i].assign(sh.vad.begin() + sh.ro[k], sh.vad.begin() + sh.ro[k + 1]);
        }
        r.all_rows[b.pos + i].assign(rows, rows + nr * r.d.row_floats);
        r.all_ns[b.pos + i] = sh.ns[k];
    }
}

void write_feature_files(Run &r, Batch &b) {
    const ctu_dims &d = r.d;
    const bool vad_files = d.has_vad && r.o.vad_out_mode != "none";
    if (vad_files)
        for (size_t i = 0; i < b.n; i++)
            if (r.items[b.pos + i].fvad.empty()) throw Fatal("VAD::new_file(): invalid filename!");
    const bool per_file = !r.ark && !r.pf;
    parallel_for(r.write_threads, b.n, [&](size_t i) {
        const Item &it = r.items[b.pos + i];
        auto [sh, k] = b.slot(i);
        if (vad_files) {  // one ASCII '0'/'1' per frame (src/vad/vad.h:67-70); NUL = nothing written (include/ctu_engine.h)
            std::vector<uint8_t> v;
            for (int64_t t = sh.ro[k]; t < sh.ro[k + 1]; t++)
                if (sh.vad[(size_t)t]) v.push_back(sh.vad[(size_t)t]);
            write_file(it.fvad, v, "FileWriter: cannot open file!");
        }
        if (per_file) {
            // -fea_trap: the reference's writers overwrite fea_kind with "spec" when they save their first frame (src/io/out.cc:182), so every header
            // after the first file carries base kind 8 (out.cc:146-152).  Not with feature files in: htkOUT::save_frame's branch for them leaves it.
            ctu_dims dh = d;
            if (r.o.fea_trap && !d.rows_in && b.pos + i > 0) dh.htk_kind = (d.htk_kind & ~077) | 8;
            auto [rows, nr] = rows_of(r, b, i);
            write_rows_out(r, it.fout, rows, nr, dh);
        }
    });
    if (!per_file)
        for (size_t i = 0; i < b.n; i++) {
            auto [rows, nr] = rows_of(r, b, i);
            if (r.ark) r.ark->add(r.items[b.pos + i].fout, rows, nr, d.row_floats);
            else r.pf->add(rows, nr, d.row_floats);
        }
}
void write_batch(Run &r, Batch &b) {
    if (r.o.verbose)
        for (size_t i = 0; i < b.n; i++) {
            auto [sh, k] = b.slot(i);
            std::fprintf(stderr, "processing: %s - %lld frames.\n", r.items[b.pos + i].fin.c_str(), (long long)(r.signal_out ? sh.ro[k + 1] - sh.ro[k] : sh.kept[k]));
        }
    if (r.signal_out) write_signal_files(r, b);
    else if (r.cmvn) stash_for_cmvn(r, b);
    else write_feature_files(r, b);
}

void write_batches(Run &r, BatchChan &to_writer, std::atomic<bool> &giving_up, std::exception_ptr &err) {
    std::unique_ptr<Batch> b;
    while (!err && to_writer.pop(b)) {
        const double t0 = now();
        try {
            write_batch(r, *b);
        } catch (...) {
            err = std::current_exception();
            giving_up = true;
        }
        b.reset();  // its buffers go back to the pool
        r.t_write += now() - t0;
    }
    to_writer.close();  // a failed writer must not leave the engines waiting to hand over
}
// ---- the pipeline: reader -> engines (this thread) -> writer, one batch in each at a time
void run_pipeline(Run &r) {
    const bool timing = std::getenv("CTU_HOST_TIMING") != nullptr;  // the stages' busy seconds on stderr at the end
    const double t_loop0 = now();
    BatchChan to_engine(1), to_writer(1);
    std::atomic<bool> giving_up{false};
    std::exception_ptr writer_err, engine_err;
    {
        StageThreads<BatchChan> th{to_engine, to_writer, {}, {}};
        th.reader = std::thread([&] { read_batches(r, to_engine, giving_up); });
        th.writer = std::thread([&] { write_batches(r, to_writer, giving_up, writer_err); });
        std::unique_ptr<Batch> b;
        while (!engine_err && to_engine.pop(b)) {
            if (b->err) {
                engine_err = b->err;
                break;
            }
            const double t0 = now();
            try {
                run_batch(r, *b);
            } catch (...) {
                engine_err = std::current_exception();
                break;
            }
            r.t_engine += now() - t0;
            if (!to_writer.push(std::move(b))) break;
        }
        giving_up = giving_up || (bool)engine_err;
    }  // th: a reader blocked on a full hand-over sees the close, both threads are joined; a batch still queued dies with its channel
    if (timing)
        std::fprintf(stderr, "host stages busy: reader %.3f s, engines %.3f s, writer %.3f s; loop %.3f s, %d + %d I/O threads, %d engine(s)\n", r.t_read, r.t_engine,
                     r.t_write, now() - t_loop0, r.io_threads, r.write_threads, r.ngpu);
    if (writer_err) std::rethrow_exception(writer_err);
    if (engine_err) std::rethrow_exception(engine_err);
}
// speaker table in order of first appearance (cmvn_POST::add_spk, src/fea/post_impl.cc:120-142): the names; `of` = every item's speaker
std::vector<std::string> speaker_table(const std::vector<Item> &items, std::vector<int32_t> &of) {
    std::vector<std::string> names;
    std::unordered_map<std::string, int32_t> index;
    for (const Item &it : items) {
        auto ins = index.emplace(it.spk, (int32_t)names.size());
        if (ins.second) names.push_back(it.spk);
        of.push_back(ins.first->second);
    }
    return names;
}
// shards over the whole corpus; every GPU keeps its rows in one block behind a plan with the same geometry
struct CorpusShard {
    std::vector<size_t> idx;
    std::vector<int32_t> spk;
    std::vector<float> rows;
    Plan plan;
};
std::vector<CorpusShard> shard_corpus(Run &r, const std::vector<int32_t> &spk_of) {
    std::vector<CorpusShard> sh(r.ngpu);
    std::vector<size_t> load(r.ngpu, 0);
    for (size_t i = 0; i < r.items.size(); i++) {
        const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        sh[g].idx.push_back(i);
        load[g] += r.all_rows[i].size();
    }
    for (int g = 0; g < r.ngpu; g++) {
        std::vector<int64_t> ns;
        for (size_t i : sh[g].idx) {
            ns.push_back(r.all_ns[i]);
            sh[g].spk.push_back(spk_of[i]);
            sh[g].rows.insert(sh[g].rows.end(), r.all_rows[i].begin(), r.all_rows[i].end());
            std::vector<float>().swap(r.all_rows[i]);
        }
        sh[g].plan = make_plan(r.gpus[g].eng, ns);
    }
    return sh;
}
// one pass over every GPU's rows, partial sums added on the host; per speaker and column, the sum over the count less `less`:
// the mean (mean = NULL, less = 0: sum_fea + stat_cm, post_impl.cc:51-76), then the variance about it (less = 1: sum_cv + stat_cv, :78-102)
std::vector<double> cmvn_moment(Run &r, std::vector<CorpusShard> &sh, int n_spk, int cols, const double *mean, int less) {
    std::vector<double> acc((size_t)n_spk * (cols + 1), 0.0), out((size_t)n_spk * cols);
    std::vector<std::vector<double>> part(r.ngpu, acc);
    per_gpu(r.ngpu, [&](int g) {
        if (sh[g].idx.empty()) return;
        if (ctu_cmvn_accumulate_host(r.gpus[g].eng, sh[g].plan.get(), sh[g].rows.data(), sh[g].spk.data(), n_spk, mean, part[g].data()) != CTU_OK)
            throw Fatal(ctu_last_error(r.gpus[g].eng));
    });
    for (int g = 0; g < r.ngpu; g++)
        for (size_t k = 0; k < acc.size(); k++) acc[k] += part[g][k];
    for (int s_ = 0; s_ < n_spk; s_++)
        for (int k = 0; k < cols; k++) out[(size_t)s_ * cols + k] = acc[(size_t)s_ * (cols + 1) + k] / (acc[(size_t)s_ * (cols + 1) + cols] - less);
    return out;
}
// cmvnOUT::save_frame (src/io/out.cc:591-613)
void write_cmvn_stats(const std::string &path, const std::vector<std::string> &names, int cols, const std::vector<double> &mean, const std::vector<double> &var) {
    FILE *f = std::fopen(path.c_str(), "wt");
    if (!f) throw Fatal("OUT: Cannot create output file with stat. of cmvn!");
    for (size_t s_ = 0; s_ < names.size(); s_++) {
        std::fprintf(f, "%s\nmean\t", names[s_].c_str());
        for (int k = 0; k < cols; k++) std::fprintf(f, k + 1 < cols ? "%f " : "%f", mean[s_ * cols + k]);
        std::fprintf(f, "\nvar\t");
        for (int k = 0; k < cols; k++) std::fprintf(f, k + 1 < cols ? "%f " : "%f\n", var[s_ * cols + k]);
    }
    std::fclose(f);
}
// What BATCH::save_frame does with the normalised vectors of file i (src/io/batch.cc:230-241): through the majority filter's ring - whose
// index the previous files of the list have left somewhere (include/ctu_engine.h) -, the decision, the drop.  The energy column does not go
// through the ring (the engine has already moved it to the row the writer reads it with).  `rows`: the file's T normalised rows in, the rows
// it writes out (they live in vr.vrows); their number is returned.
struct VadRing {
    int32_t hidx = 0, hsize = 0;  // the majority filter along the list (the apply pass is the only one that pushes into it)
    std::vector<float> vrows;
    std::vector<int32_t> src;
};
int64_t vad_on_normalised_rows(const Run &r, size_t i, VadRing &vr, const float *&rows, int64_t T) {
    const ctu::Opts &o = r.o;
    const int64_t D = r.d.row_floats;
    const int e_col = o.fea_E ? (int)D - 1 : -1;
    vr.src.assign((size_t)std::max<int64_t>(T, 1), -1);
    if (vr.hsize != 0) throw half_drained(r, i - 1);
    const int64_t n_out = ctu_vad_ring_rows(o.vad_filter_order, T, vr.hidx, vr.src.data());
    ctu_vad_ring_step(o.vad_filter_order, T, &vr.hidx, &vr.hsize);
    const std::vector<uint8_t> &v = r.all_vads[i];
    std::vector<uint8_t> dec;
    vr.vrows.clear();
    for (int64_t q = 0; q < n_out; q++) {
        const uint8_t b = v[(size_t)q];
        if (b) dec.push_back(b);
        if (o.vad_apply_mode == "drop" && b != '1') continue;
        const size_t at = vr.vrows.size();
        vr.vrows.resize(at + (size_t)D, 0.f);
        for (int c = 0; c < (int)D; c++) {
            if (c == e_col) vr.vrows[at + c] = rows[(size_t)q * D + c];
            else if (vr.src[(size_t)q] >= 0) vr.vrows[at + c] = rows[(size_t)vr.src[(size_t)q] * D + c];
        }
    }
    if (o.vad_out_mode != "none") {
        if (r.items[i].fvad.empty()) throw Fatal("VAD::new_file(): invalid filename!");
        write_file(r.items[i].fvad, dec, "FileWriter: cannot open file!");
    }
    rows = vr.vrows.data();
    return (int64_t)(vr.vrows.size() / (size_t)D);
}
// the third pass: normalise on the GPUs, then back to list order and the writers
void cmvn_apply_and_write(Run &r, std::vector<CorpusShard> &sh, int n_spk, const std::vector<double> &mean, const std::vector<double> &var) {
    per_gpu(r.ngpu, [&](int g) {
        if (sh[g].idx.empty()) return;
        if (ctu_cmvn_apply_host(r.gpus[g].eng, sh[g].plan.get(), sh[g].rows.data(), sh[g].spk.data(), n_spk, mean.data(), var.data()) != CTU_OK)
            throw Fatal(ctu_last_error(r.gpus[g].eng));
    });
    std::vector<std::pair<int, size_t>> where(r.items.size());  // (gpu, position in that GPU's shard)
    for (int g = 0; g < r.ngpu; g++)
        for (size_t k = 0; k < sh[g].idx.size(); k++) where[sh[g].idx[k]] = {g, k};
    VadRing vr;
    for (size_t i = 0; i < r.items.size(); i++) {
        const CorpusShard &s = sh[where[i].first];
        const size_t k = where[i].second;
        const int64_t *ro = ctu_plan_row_offsets(s.plan.get());
        int64_t nr = ro[k + 1] - ro[k];
        const float *rows = s.rows.data() + (size_t)ro[k] * r.d.row_floats;
        if (r.cmvn_vad) nr = vad_on_normalised_rows(r, i, vr, rows, nr);
        if (r.ark) r.ark->add(r.items[i].fout, rows, nr, r.d.row_floats);
        else if (r.pf) r.pf->add(rows, nr, r.d.row_floats);
        else write_rows_out(r, r.items[i].fout, rows, nr, r.d);
    }
}

void cmvn_pass(Run &r, const std::string &stat_path) {
    std::vector<int32_t> spk_of;
    const std::vector<std::string> spk_names = speaker_table(r.items, spk_of);
    const int n_spk = (int)spk_names.size(), cols = ctu_cmvn_cols(r.gpus[0].eng);
    std::vector<CorpusShard> sh = shard_corpus(r, spk_of);
    const std::vector<double> mean = cmvn_moment(r, sh, n_spk, cols, nullptr, 0), var = cmvn_moment(r, sh, n_spk, cols, mean.data(), 1);
    write_cmvn_stats(stat_path, spk_names, cols, mean, var);
    if (!r.o.apply_cmvn && r.cmvn_vad && r.o.vad_out_mode != "none")  // statistics only: VAD::new_file still opens every file's VAD output
        for (const Item &it : r.items)
            if (!it.fvad.empty()) write_file(it.fvad, std::vector<uint8_t>(), "FileWriter: cannot open file!");
    if (r.o.apply_cmvn) cmvn_apply_and_write(r, sh, n_spk, mean, var);
}

// -online_in: the whole run.  What no stream set takes is refused ahead of the engine and of the first byte of input, in the set's words.
int pipe_stage(Run &r) {
    const ctu::Opts &o = r.o;
    if (o.format_out == "ark" || o.format_out == "pfile")
        throw Fatal("ENGINE: online input: -format_out " + o.format_out + " (an archive is written for a list; a pipe writes htk, raw or wave)");
    r.pipe_drop = o.do_vad() && o.vad_apply_mode == "drop";
    std::vector<const char *> cargs;
    for (auto &a : r.args) cargs.push_back(a.c_str());
    if (r.pipe_drop) {
        cargs.push_back("-vad_apply_mode");
        cargs.push_back("none");
    }
    PipeJob job;
    char reason[1024];
    const int rc = ctu_streams_flags_for((int)cargs.size(), cargs.data(), &job.flags, reason, sizeof reason, &job.halo);
    if (rc == CTU_ERR_OPTS) throw Fatal(reason);
    if (rc != CTU_OK) {
        const std::string why(reason), lead("ENGINE: ");
        throw Fatal("ENGINE: online input: " + (why.compare(0, lead.size(), lead) == 0 ? why.substr(lead.size()) : why));
    }
    (void)PipeDecoder(o);  // (an input format outside raw | alaw | mulaw | wave: the reader's words)
    if (o.do_vad() && o.vad_out_mode != "none") {
        if (o.vad_out.empty()) throw Fatal("VAD::new_file(): invalid filename!");
        job.vad_path = o.vad_out;
    }
    if (r.ngpu > 1 && o.verbose) std::fprintf(stderr, "ENGINE: online input is one stream: running on one GPU\n");
    r.ngpu = 1;
    if (!r.gpu_map.empty()) r.gpu_map.resize(1);
    make_engines(r);
    job.eng = r.gpus[0].eng;
    job.read_bytes = r.pipe_read_bytes;
    job.drop = r.pipe_drop;
    const int64_t frames = run_pipe(job, o, r.d);
    if (o.verbose) std::fprintf(stderr, "processing: <stdin> - %lld frames.\n", (long long)frames);
    return 0;
}

int real_main(int argc, char **argv) {
    Run r;
    parse_host_flags(r, argc, argv);
    ctu::Opts &o = r.o;
    try {
        o = ctu::Opts::from_args(r.args);
    } catch (const ctu::OptsError &e) {
        if (r.args.empty()) std::fputs(ctu::Opts().usage().c_str(), stderr);
        throw Fatal(e.what());
    }
    if (o.help) {
        std::fputs(o.usage().c_str(), stdout);
        return 0;
    }
    r.signal_out = o.format_out == "raw" || o.format_out == "wave";
    if (!r.signal_out && o.format_out != "htk" && o.format_out != "ark" && o.format_out != "pfile") throw Fatal("OUT: Unknown output file format!");
    // --channels: refused ahead of the engine and of any input where a file is not N channels of samples
    if (r.channels > 1 && o.pipe_in) throw Fatal("ENGINE: --channels above 1 with -online_in (a pipe is one stream: one set of streams per pipe is not built)");
    if (r.channels > 1 && o.pipe_out) throw Fatal("ENGINE: --channels above 1 with -online_out (a pipe takes one file, --channels writes one per channel)");
    if (r.channels > 1 && o.format_in == "htk") throw Fatal("ENGINE: --channels above 1 with -format_in htk (a feature file has rows, not channels)");
    r.items = expand_channels(read_items(o), r.channels);
    if (o.pipe_in) return pipe_stage(r);
    r.wire_format = wire_format_of(o.format_in, o.swap_in, r.channels);
    // a WAVE header says how many channels it holds: the list's first file is asked ahead of the engine, so a wrong --channels (or a file
    // that is not mono without it) needs no device to be told; the files behind it are asked where they always were (size_batch)
    if (o.format_in == "wave" && !r.items.empty()) (void)probe_samples(o, r.items[0].fin, r.channels);
    // hwss / fwss / 2fwss chain the list through the noise seed (src/nr/nr.cc:212-221): one GPU, files in list order
    const bool chained = o.nr_mode == "hwss" || o.nr_mode == "fwss" || o.nr_mode == "2fwss";
    if (chained && r.ngpu > 1) {
        if (o.verbose) std::fprintf(stderr, "ENGINE: -nr_mode %s chains the files of the list: running on one GPU\n", o.nr_mode.c_str());
        r.ngpu = 1;
    }
    r.cmvn = o.stat_cmvn || o.apply_cmvn;
    r.cmvn_vad = r.cmvn && o.do_vad();
    make_engines(r);
    const std::string deferred_error = chained && o.vadmode == "file" ? cut_at_end_of_vad_stream(r) : "";
    open_writers(r);
    const std::string stat_path = cmvn_stat_path(o);
    r.all_rows.resize(r.cmvn ? r.items.size() : 0);
    r.all_ns.resize(r.cmvn ? r.items.size() : 0);
    r.all_vads.resize(r.cmvn_vad ? r.items.size() : 0);
    // The reference's VAD keeps its majority filter for the whole list and cleanFilter() does not reset its ring index between files
    // (src/vad/vad.h:110-121): the rows of a file depend on the frame counts of the files in front of it (include/ctu_engine.h).
    r.vad_ring = r.d.has_vad && o.vad_filter_order > 1 && !r.cmvn_vad;  // with CMVN the ring acts on the normalised rows: cmvn_pass
    run_pipeline(r);
    if (!deferred_error.empty()) throw Fatal(deferred_error);
    if (r.cmvn) cmvn_pass(r, stat_path);
    if (r.pf) r.pf->close();
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        return real_main(argc, argv);
    } catch (const std::exception &e) {  // the reference prints the thrown text and returns -1 (src/main.cpp:54-60)
        std::fprintf(stderr, "%s\n", e.what());
        return -1;
    }
}
