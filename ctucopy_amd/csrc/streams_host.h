// Streaming input (include/ctu_engine.h: ctu_streams_*), host side: the stream set, its creation, pushes and finishes.
// Included by engine.hip inside its extern "C" block, behind everything a run is made of (one translation unit).
//
// What a set is - its kinds of state, halo, strides, the size of every buffer - is stream_set_shape's to say (stream_set_shape.h, host only,
// also compiled and tested without HIP): ctu_streams_create_ex refuses, takes the shape, creates the set's plan and allocates by the shape.
//
// A push is check, plan, commit, launch, and every push is push_common.  The checks refuse ahead of everything else.  stream_plan_push
// (stream_plan.h, host only, also compiled and tested without HIP) then lays the whole push out from the set's mirrors without touching them.
// The commit copies the mirrors' next values into the set, and from there on a push is HIP calls alone, sized by the plan (two HIP calls come
// ahead of the plan: the device is selected, and the plan waits for this turn's page-locked descriptors, which it writes, to be free): the
// run goes over the front of the set's ctu_plan with the extent of the push (RunExtent), so the plan itself is not written after create.
// Between the stitch and the carry a set with rows out runs push_rows: on a set with detector state the run stops ahead of the VAD's
// sequential stages (run_chain: vad_stages off) and launch_stream_vad replays them from the set's own state, by the plan's RowPush
// descriptors and its list of the streams that complete a frame.  With CTU_STREAMS_VAD_ROW_STATE beside the row and the detector state
// (sh.vad_rows) launch_stream_vad_rows makes the calls of the push behind the chain's delay (the plan's VadCalls, the criterion record)
// and the row kernels deliver the rows that leave h calls behind theirs.  A set with signal state (speech output) runs push_signal: the run leaves
// the time-domain frames of the push in the plan's ybuf and stream_ola_kernel adds them onto every stream's tail of the overlap-add
// (stream_signal_kernels.h).
// A HIP call that fails behind the commit (CTU_ERR_DEVICE) leaves mirrors and device state out of step: include/ctu_engine.h says what
// the caller may still do with the set.
#pragma once

static_assert(SHAPE_OLA_TAIL_MAX == OLA_TAIL_MAX && SHAPE_OLA_BIG_TAIL_MAX == OLA_BIG_TAIL_MAX && SHAPE_STREAM_MEANS == STREAM_MEANS,
              "stream_set_shape.h restates the stream kernels' limits");

extern "C++" {
// Descriptors that travel with a push: two page-locked buffers and their device copies, used in turn (ctu_streams::turn, desc_free)
template <class T>
struct TurnBuf {
    T *h[2] = {nullptr, nullptr};
    DevBuf<T> d[2];
    void alloc(size_t n) {
        for (int k = 0; k < 2; k++) {
            h[k] = static_cast<T *>(ctu_host_alloc(n * sizeof(T)));
            if (!h[k]) throw std::runtime_error("page-locked descriptors of a stream set");
            d[k].alloc(n);
        }
    }
    void upload(int k, size_t count, hipStream_t s) { HIP_TRY(hipMemcpyAsync(d[k].p, h[k], count * sizeof(T), hipMemcpyHostToDevice, s)); }
    ~TurnBuf() {
        for (T *p : h) ctu_host_free(p);
    }
};
}

// A stream set (ctu_streams_create): per-stream state in HBM, and what a push needs that does not change from push to push - a plan over
// n_streams utterances of the longest stitched length (its HostPlan, plan_host.h, is where the set reads the arena size, the tile and row
// totals from), whose tile list, chain heads (workgroup g starts at tile g), arena and scratch a push uses the front of.  The tile records themselves are written by stream_stitch_kernel, push after push.
struct ctu_streams {
    ctu_engine *eng = nullptr;
    int64_t max_push = 0;
    StreamSetShape sh;               // what the set is; sh.g: what stream_plan_push lays a push out by
    std::unique_ptr<const ctu_plan> plan;  // (const: a push runs the front of it by a RunExtent of its own, nothing writes it after create)
    DevBuf<int16_t> arena, carry;
    DevBuf<StreamState> state;
    std::vector<int64_t> consumed;   // the host's mirror of StreamState::consumed: layout and row counts of a push need no copy back
    std::vector<int64_t> next_consumed;  // (of the push at hand, by position in it: PushLayout::consumed)
    std::vector<int64_t> counts;         // (PushLayout::row_counts of a push whose caller passes no array; the host form reads them here)
    std::vector<uint32_t> seen;      // the push a stream was last named in (a repeat inside one push is refused)
    uint32_t push_no = 0;
    TurnBuf<StreamPush> desc;        // the descriptors of a push, each turn guarded by the event behind its last reader
    hipEvent_t desc_free[2] = {nullptr, nullptr};
    int turn = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around stream_stitch_kernel and stream_carry_kernel of the last push
    bool timed = false;
    // CTU_STREAMS_ROW_STATE with a delta chain, stacking or CMS (stream_rows_kernels.h; sh.g.held, H, wmax): the two histories of every
    // stream (sh.C rows of sh.hw floats) and which one is current, the running means, the descriptors of the row kernels
    DevBuf<float> hist, means;
    std::vector<uint8_t> hsel, next_hsel;
    TurnBuf<RowPush> rdesc;
    // CTU_STREAMS_NR_STATE on a chain with -nr_mode exten (sh.chained): Navg | Yavg of every stream (frontend_kernel<..., XS>; with
    // CTU_STREAMS_LARGE_STATE on 1024 .. 4096 points wave1k_kernel<true, XS> / bigfft_kernel<NIT, true, XS>), the heads of the chains a push is
    // dealt onto, and the stream of every tile.  CTU_STREAMS_SS_STATE on a chain with -nr_mode hwss | fwss | 2fwss: the same buffer and the
    // same chains, a slot of xs_ss_floats per stream - Navg | Nravg and the detector's record (frontend_kernel<..., SS, ..., XS>); with
    // CTU_STREAMS_SS_SIGNAL_STATE on speech output the same slots beside the tails below (frontend_kernel<..., SS, SY, ..., XS>); with
    // CTU_STREAMS_SS_LARGE_STATE on 2048- / 4096-point frames a slot of xs_ss_big_floats per stream, all in 8-byte cells - Navg | Nravg as
    // doubles and the detector's record (bigss_kernel<NIT, true>, ss_decide_stream_kernel), on workgroup chains as bigfft_kernel's
    DevBuf<float> xstate;
    TurnBuf<int> heads;
    std::vector<int> chain_tail;     // (scratch of stream_plan_push)
    // CTU_STREAMS_VAD_STATE on a configuration with the VAD module (stream_vad_kernels.h; sh.vad, H = h, wmax = h - 1): the detector's
    // record of every stream, the base rows of a push ahead of their delayed copy (h > 0: the histories above hold the last h of them),
    // the decisions of a push nobody asked for (and of the host forms, ahead of the download), the streams of a push that run the replay
    DevBuf<double> vstate;
    DevBuf<float> vbase;
    DevBuf<uint8_t> vsink;
    TurnBuf<int> replay;
    // CTU_STREAMS_VAD_ROW_STATE beside the row and the detector state, the VAD module with a chain, a stacking or CMS behind it (sh.vad_rows;
    // sh.g.H, wmax the chain's, sh.g.vh = h): the histories hold h more base rows, from which the rows held back are rebuilt (vbase is not
    // used); the criterion input of every stream's newest frame, and the calls of a push's streams (stream_vad_delayed_kernel)
    DevBuf<double> crec;
    TurnBuf<VadCalls> vcalls;
    // CTU_STREAMS_SIGNAL_STATE on a configuration with speech output (stream_signal_kernels.h; sh.signal): the overlap-add's tail of every
    // stream - sh.tstride doubles each, window - wshift of them in use - and the descriptors of stream_ola_kernel / stream_ola_big_kernel
    DevBuf<double> otail;
    TurnBuf<SignalPush> sdesc;
    // CTU_STREAMS_TRAP_STATE on a configuration with -fea_kind trapdct (stream_trap_kernels.h; sh.trap, H = half, wmax = half - 1): the
    // histories above hold the last C = 2 half log-mel rows of every stream; the stream of every column of stream_trap_kernel
    TurnBuf<int> cols;
    // the host form: page-locked staging of the new samples, their device copy, the rows (the samples) ahead of the download
    int16_t *h_stage = nullptr;
    DevBuf<int16_t> d_stage;
    DevBuf<float> d_rows;
    DevBuf<int16_t> d_sig;
    std::vector<int64_t> offs;
    ~ctu_streams() {
        ctu_host_free(h_stage);
        for (hipEvent_t v : desc_free)
            if (v) (void)hipEventDestroy(v);
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
    }
};

int ctu_streams_config_check(int argc, const char *const *argv, char *reason, int64_t cap) {
    return ctu_streams_config_check_ex(argc, argv, 0, reason, cap, nullptr);
}

int ctu_streams_config_check_ex(int argc, const char *const *argv, uint32_t flags, char *reason, int64_t cap, int32_t *halo) {
    if (halo) *halo = 0;
    auto say = [&](const std::string &m) {
        g_create_error = m;
        if (reason && cap > 0) {
            std::strncpy(reason, m.c_str(), (size_t)cap - 1);
            reason[cap - 1] = 0;
        }
    };
    say("");
    try {
        ctu::Opts o = ctu::Opts::from_args(to_args(argc, argv));
        ctu::Design d(o);
        spread_small_fft(d);
        std::string why;
        if (const int rc = streams_check(d, flags, why)) {
            say(why);
            return rc;
        }
        int H = 0, wmax = 0;
        stream_set_halo(d, flags, &H, &wmax);
        if (halo) *halo = H;
        return CTU_OK;
    } catch (const std::exception &ex) {
        say(ex.what());
        return CTU_ERR_OPTS;
    }
}

int ctu_streams_flags_for(int argc, const char *const *argv, uint32_t *flags, char *reason, int64_t cap, int32_t *halo) {
    uint32_t need = 0;
    try {
        ctu::Design d(ctu::Opts::from_args(to_args(argc, argv)));
        spread_small_fft(d);
        need = ctu::streams_flags_for(d);
    } catch (const std::exception &) {  // (a bad command line: the check below says the parser's words)
    }
    if (flags) *flags = need;
    return ctu_streams_config_check_ex(argc, argv, need, reason, cap, halo);
}

int64_t ctu_streams_step(int32_t window, int32_t wshift, int64_t total, int64_t *carry) {
    if (!stream_step_args_ok(window, wshift, total)) return CTU_ERR_INPUT;
    const int64_t F = stream_frames(total, window, wshift);
    if (carry) *carry = total - F * wshift;
    return F;
}

int64_t ctu_streams_rows_step(int32_t window, int32_t wshift, int32_t halo, int32_t wmax, int64_t total, int64_t *pending) {
    // (a chain's largest window is at least 1; trapdct's rule is wmax = halo - 1, which is 0 for a context of three frames)
    if (!stream_step_args_ok(window, wshift, total) || halo < 0 || wmax < 0 || wmax > halo || (halo > 0 && wmax < 1 && wmax != halo - 1)) return CTU_ERR_INPUT;
    return stream_rows_step(window, wshift, halo, wmax, total, pending);
}

int64_t ctu_streams_vad_step(int32_t window, int32_t wshift, int32_t filter_order, int64_t total, int64_t *pending) {
    if (!stream_step_args_ok(window, wshift, total) || filter_order < 1 || filter_order > 31) return CTU_ERR_INPUT;
    int H = 0, wmax = 0;
    stream_vad_halo(filter_order, &H, &wmax);
    return stream_rows_step(window, wshift, H, wmax, total, pending);
}

int64_t ctu_streams_vad_rows_step(int32_t window, int32_t wshift, int32_t filter_order, int32_t halo, int32_t wmax, int64_t total, int64_t *pending) {
    // (the arguments of the two calls above, each with its own rule)
    if (ctu_streams_rows_step(window, wshift, halo, wmax, total, nullptr) < 0 || filter_order < 1 || filter_order > 31) return CTU_ERR_INPUT;
    return stream_vad_rows_step(window, wshift, (filter_order - 1) / 2, halo, wmax, total, pending);
}

int64_t ctu_streams_signal_step(int32_t window, int32_t wshift, int64_t total, int64_t *pending) {
    if (!stream_step_args_ok(window, wshift, total)) return CTU_ERR_INPUT;
    return stream_signal_step(window, wshift, total, pending);
}

int ctu_streams_create(ctu_engine *e, int32_t n_streams, int64_t max_push_samples, ctu_streams **out) {
    return ctu_streams_create_ex(e, n_streams, max_push_samples, 0, out);
}

int ctu_streams_create_ex(ctu_engine *e, int32_t n_streams, int64_t max_push_samples, uint32_t flags, ctu_streams **out) {
    if (!e || !out) return CTU_ERR_INPUT;
    *out = nullptr;
    // ---- refuse
    if (ctu::streams_flags_unknown(flags)) {
        set_error(e, "ENGINE: unknown stream set flags");
        return CTU_ERR_INPUT;
    }
    if (n_streams < 1 || max_push_samples < 1 || max_push_samples > (1 << 26)) {
        set_error(e, "ENGINE: a stream set needs at least one stream and pushes of 1 .. 2^26 samples");
        return CTU_ERR_INPUT;
    }
    const ctu::Design &d = *e->design;
    if (const std::string why = streams_unsupported_reason(d, flags); !why.empty()) {
        set_error(e, "ENGINE: configuration cannot be streamed: " + why);
        return CTU_ERR_UNSUPPORTED;
    }
    // ---- the shape
    StreamSetFacts f;
    f.ss = e->tab.ss; f.big = e->tab.big; f.ss_file = e->tab.ss_file; f.wave1k = e->tab.path == BIG_WAVE1K; f.mode = e->tab.sel.mode;
    f.per_wave = e->geom.per_wave; f.chain_slots = e->geom.chain_slots; f.max_wg = e->geom.max_wg;
    std::unique_ptr<ctu_streams> st(new ctu_streams);
    st->eng = e;
    st->max_push = max_push_samples;
    StreamSetShape &sh = st->sh;
    sh = stream_set_shape(d, flags, f, n_streams, max_push_samples);
    if (sh.refusal) {
        set_error(e, std::string("ENGINE: ") + sh.refusal);
        return CTU_ERR_UNSUPPORTED;
    }
    // ---- the plan, of n_streams longest slots
    const std::vector<int64_t> longest((size_t)n_streams, sh.longest);
    ctu_plan *pl = nullptr;
    if (const int rc = ctu_plan_create(e, longest.data(), n_streams, &pl); rc != CTU_OK) return rc;
    st->plan.reset(pl);
    sh.g.arena_samples = pl->hp.total_samples;
    sh.g.tile_cap = (int64_t)pl->hp.tiles.size();
    // ---- allocate and zero by the shape.  The mirrors, and what a planned push is written into: a push allocates nothing
    for (auto *v : {&st->consumed, &st->next_consumed, &st->counts, &st->offs}) v->assign((size_t)n_streams, 0);
    for (auto *v : {&st->hsel, &st->next_hsel}) v->assign((size_t)n_streams, 0);
    st->seen.assign((size_t)n_streams, 0);
    if (sh.chained) st->chain_tail.assign((size_t)sh.n_heads, -1);
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const int64_t tf = pl->hp.total_frames;
        auto zeroed = [](auto &buf, size_t n) {
            buf.alloc(n);
            HIP_TRY(hipMemset(buf.p, 0, n * sizeof(*buf.p)));
        };
        zeroed(st->arena, (size_t)pl->hp.total_samples);
        zeroed(st->carry, (size_t)n_streams * sh.cstride);
        zeroed(st->state, (size_t)n_streams);
        st->desc.alloc((size_t)n_streams);
        for (hipEvent_t &v : st->desc_free) HIP_TRY(hipEventCreateWithFlags(&v, hipEventDisableTiming));
        if (sh.g.held || sh.vad) st->rdesc.alloc((size_t)n_streams);
        if (sh.chained) {
            zeroed(st->xstate, (size_t)n_streams * (size_t)sh.xstate_floats);  // (never read ahead of a store: a file's first tile resets)
            zeroed(pl->tile_utt, pl->tiles.n);
            st->heads.alloc((size_t)sh.n_heads);
        }
        if (sh.vad) {
            zeroed(st->vstate, (size_t)n_streams * VST_DOUBLES);  // (never read ahead of a store: a file's first push resets)
            st->vsink.alloc((size_t)sh.vsink_n(tf));
            st->vbase.alloc((size_t)sh.vbase_n(tf));
            st->replay.alloc((size_t)n_streams);
            if (sh.vad_rows) {
                zeroed(st->crec, (size_t)sh.crec_n());  // (never read ahead of a store: a call reads frames of the file)
                st->vcalls.alloc((size_t)n_streams);
            }
        }
        if (sh.signal) {
            zeroed(st->otail, (size_t)sh.otail_n());  // (+0.0: a file's first frames add to nothing)
            st->sdesc.alloc((size_t)n_streams);
        }
        if (sh.g.held) {
            zeroed(st->hist, (size_t)sh.hist_n());
            zeroed(st->means, (size_t)sh.means_n());
        }
        if (sh.trap) st->cols.alloc((size_t)sh.cols_n(tf));
        for (hipEvent_t &v : st->ev) HIP_TRY(hipEventCreate(&v));
        return CTU_OK;
    });
    if (rc != CTU_OK) return rc;
    *out = st.release();
    return CTU_OK;
}

void ctu_streams_destroy(ctu_streams *st) {
    if (!st) return;
    (void)hipSetDevice(st->eng->device);
    (void)hipDeviceSynchronize();  // pushes may still be in flight on the caller's streams
    delete st;
}

int64_t ctu_streams_frames(const ctu_streams *st, int32_t id) {
    if (!st || id < 0 || id >= st->sh.n_streams) return CTU_ERR_INPUT;
    return stream_vad_rows_step(st->sh.g.window, st->sh.g.wshift, st->sh.g.vh, st->sh.g.H, st->sh.g.wmax, st->consumed[(size_t)id], nullptr);
}

int64_t ctu_streams_pending(const ctu_streams *st, int32_t id) {
    if (!st || id < 0 || id >= st->sh.n_streams) return CTU_ERR_INPUT;
    int64_t pending = 0;
    st->sh.delivered(st->consumed[(size_t)id], &pending);
    return pending;
}

namespace {
// The row kernels of a push, or of a finish, over the n streams rdesc.h[k] describes (uploaded here); `most` is the largest row count among them
void launch_stream_rows(ctu_streams *st, int k, int n, int64_t most, bool finishing, float *d_rows, hipStream_t s, bool upload = true) {
    const ctu::Design &d = *st->eng->design;
    if (upload) st->rdesc.upload(k, (size_t)n, s);
    if (most == 0) return;
    RowParams rp;
    rp.push = st->rdesc.d[k].p; rp.fresh = st->plan->base_rows.p; rp.hist = st->hist.p; rp.means = st->means.p; rp.rows = d_rows;
    rp.n_streams = st->sh.n_streams; rp.C = st->sh.C; rp.Dbase = d.Dbase; rp.finishing = finishing ? 1 : 0;
    const unsigned chunks = (unsigned)((most + 63) / 64);
    if (d.post_order > 0) {
        size_t shm = 0;
        const PostParams pp = post_params(d, &shm);
        if (d.post_stack) hipLaunchKernelGGL(stream_post_kernel<true>, dim3(chunks, (unsigned)n), dim3(256), shm, s, rp, pp);
        else hipLaunchKernelGGL(stream_post_kernel<false>, dim3(chunks, (unsigned)n), dim3(256), shm, s, rp, pp);
    }
    if (d.cms) {
        const CmsParams cp = cms_params(d);
        if (d.cms == 1) hipLaunchKernelGGL(stream_cms_exp_kernel, dim3((unsigned)n), dim3(64), 0, s, rp, cp);
        else hipLaunchKernelGGL(stream_cms_block_kernel, dim3(chunks, (unsigned)n), dim3(256), (size_t)(64 + cp.L - 1) * cp.ncols * sizeof(float), s, rp, cp);
    }
    HIP_TRY(hipGetLastError());
}
// stream_trap_kernel over the rows that go out with a push, or with a finish, of the n streams rdesc.h[k] describes (uploaded here, with
// the stream of every column)
void launch_stream_trap(ctu_streams *st, int k, int n, float *d_rows, hipStream_t s) {
    const ctu::Design &d = *st->eng->design;
    st->rdesc.upload(k, (size_t)n, s);
    const int64_t n_cols = stream_trap_columns(st->rdesc.h[k], n, st->cols.h[k]);
    if (n_cols == 0) return;
    st->cols.upload(k, (size_t)n_cols, s);
    StreamTrapParams tp;
    tp.push = st->rdesc.d[k].p; tp.col = st->cols.d[k].p; tp.fresh = st->plan->logmel.p; tp.hist = st->hist.p; tp.G = st->eng->trapG.p; tp.rows = d_rows;
    tp.n_cols = n_cols; tp.n_streams = st->sh.n_streams; tp.C = st->sh.C; tp.B = d.B;
    tp.traplen = d.o.fea_trapdct_traplen; tp.ndct = d.o.fea_trapdct_ndct; tp.D = d.D;
    const int nrb = tp.ndct <= 16 ? 1 : 2, bb = nrb == 1 ? 8 : 4;
    const dim3 grid((unsigned)((n_cols + 15) / 16), (unsigned)((d.B + bb - 1) / bb));
    const bool comp = (tp.traplen + 3) / 4 > TRAP_COMP_STEPS;  // (contexts of more than 104 frames: stream_trap_kernels.h)
    lift<1, 2>(nrb, [&](auto v) {
        lift<0, 1>(comp, [&](auto c) { hipLaunchKernelGGL((stream_trap_kernel<decltype(v)::value, decltype(c)::value != 0>), grid, dim3(64), 0, s, tp); });
    });
    HIP_TRY(hipGetLastError());
}
// The detector's kernels of a push over the n streams rdesc.h[k] describes and the L.n_replay of them replay.h[k] lists (both uploaded
// here): the replay from every stream's record, then the rows the majority filter releases with the decisions
void launch_stream_vad(ctu_streams *st, int k, int n, const PushLayout &L, float *d_rows, uint8_t *d_vad, hipStream_t s) {
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const ctu_plan *pl = st->plan.get();
    st->rdesc.upload(k, (size_t)n, s);
    if (L.n_replay == 0) return;
    st->replay.upload(k, (size_t)L.n_replay, s);
    StreamVadParams vp;
    vp.push = st->rdesc.d[k].p; vp.replay = st->replay.d[k].p; vp.n_replay = L.n_replay;
    vp.cf = pl->vad_cf.p; vp.ci = pl->vad_ci.p; vp.energy = pl->pnr.p;
    vp.vstate = st->vstate.p; vp.vad = d_vad ? d_vad : st->vsink.p;
    if (e->geom.vad_fused)
        lift<0, 1, 2, 3>(e->vp.thr, [&](auto thr) {
            hipLaunchKernelGGL((stream_vad_lanes_kernel<VF_NC, decltype(thr)::value>), dim3((unsigned)((L.n_replay + 15) / 16)), dim3(64), 0, s, vp, e->vp);
        });
    else hipLaunchKernelGGL(stream_vad_decide_kernel, dim3((unsigned)n), dim3(64), 0, s, vp, e->vp);
    if (st->sh.g.held && L.most > 0) {
        RowParams rp;
        std::memset(&rp, 0, sizeof rp);
        rp.push = st->rdesc.d[k].p; rp.fresh = st->vbase.p; rp.hist = st->hist.p; rp.rows = d_rows;
        rp.n_streams = st->sh.n_streams; rp.C = st->sh.C; rp.Dbase = d.Dbase;
        hipLaunchKernelGGL(stream_vad_rows_kernel, dim3((unsigned)((L.most + 63) / 64), (unsigned)n), dim3(256), 0, s, rp, d.D);
    }
    HIP_TRY(hipGetLastError());
}
// ... on a set with detector state behind row state: the calls of the push - the delayed replay, by the plan's VadCalls (uploaded here)
// and every stream's criterion record (with CMS alone the delay is 0 and a call reads its own frame); the fused criterion's replay as it
// stands, which only ever has CMS behind it - then the row kernels over the rows that leave h calls behind theirs
StreamVadDelay stream_vad_delay(const ctu_streams *st, const VadCalls *calls) {
    StreamVadDelay q;
    q.calls = calls; q.crec = st->crec.p; q.stride = st->sh.crec; q.delay = st->sh.g.H;
    return q;
}
void launch_stream_vad_rows(ctu_streams *st, int k, int n, const PushLayout &L, float *d_rows, uint8_t *d_vad, hipStream_t s) {
    ctu_engine *e = st->eng;
    const ctu_plan *pl = st->plan.get();
    st->rdesc.upload(k, (size_t)n, s);
    if (L.n_replay > 0) {
        StreamVadParams vp;
        vp.push = st->rdesc.d[k].p; vp.replay = st->replay.d[k].p; vp.n_replay = L.n_replay;
        vp.cf = pl->vad_cf.p; vp.ci = pl->vad_ci.p; vp.energy = pl->pnr.p;
        vp.vstate = st->vstate.p; vp.vad = d_vad ? d_vad : st->vsink.p;
        if (e->geom.vad_fused) {  // (vf_eligible: no chain, no stacking - the delay is 0)
            if (st->sh.g.H != 0) throw std::runtime_error("internal: the fused detector behind a delayed chain");
            st->replay.upload(k, (size_t)L.n_replay, s);
            lift<0, 1, 2, 3>(e->vp.thr, [&](auto thr) {
                hipLaunchKernelGGL((stream_vad_lanes_kernel<VF_NC, decltype(thr)::value>), dim3((unsigned)((L.n_replay + 15) / 16)), dim3(64), 0, s, vp, e->vp);
            });
        } else {
            st->vcalls.upload(k, (size_t)n, s);
            hipLaunchKernelGGL(stream_vad_delayed_kernel, dim3((unsigned)n), dim3(64), 0, s, vp, e->vp, stream_vad_delay(st, st->vcalls.d[k].p));
        }
        HIP_TRY(hipGetLastError());
    }
    launch_stream_rows(st, k, n, L.most, false, d_rows, s, false);
}
SignalParams signal_params(const ctu_streams *st, const SignalPush *push, int16_t *d_out) {
    const ctu::Design &d = *st->eng->design;
    SignalParams gp;
    gp.push = push; gp.ybuf = st->plan->ybuf.p; gp.tail = st->otail.p; gp.out = d_out;
    gp.tstride = st->sh.tstride; gp.window = d.window; gp.wshift = d.wshift;
    gp.corr = d.ola_corr;
    return gp;
}

int refuse(ctu_engine *e, const std::string &m) {
    set_error(e, "ENGINE: " + m);
    return CTU_ERR_INPUT;
}
// The wrong call for the set, refused before anything changes (null: the call fits the set)
const char *wrong_call(const ctu_streams *st, bool want_signal, bool want_vad, bool finish) {
    if (st->sh.signal && !want_signal)
        return "a set with signal state (CTU_STREAMS_SIGNAL_STATE) delivers samples, not rows: use ctu_streams_push_signal / ctu_streams_finish_signal";
    if (!st->sh.signal && want_signal)
        return "ctu_streams_push_signal / ctu_streams_finish_signal need a set with signal state (CTU_STREAMS_SIGNAL_STATE on a configuration with -format_out raw | wave): use ctu_streams_push / ctu_streams_finish";
    if (want_vad && !st->sh.vad)
        return finish ? "finish: decisions asked of a set without detector state (CTU_STREAMS_VAD_STATE on a configuration with the VAD module)"
                      : "push: decisions asked of a set without detector state (CTU_STREAMS_VAD_STATE on a configuration with the VAD module)";
    return nullptr;
}
// The argument checks the device and the host form of a push share (each refuses in its own words)
bool push_args_ok(const ctu_streams *st, int32_t n, const int32_t *ids, const int64_t *n_samples) { return n >= 0 && n <= st->sh.n_streams && (!n || (ids && n_samples)); }
bool push_count_ok(const ctu_streams *st, int64_t n_samples) { return n_samples >= 0 && n_samples <= st->max_push; }

// where the front end leaves the rows of a push on a set that holds rows - with trap state its log-mel rows, and no kernel of the run writes rows
float *held_base(const ctu_streams *st) { return st->sh.trap ? st->plan->logmel.p : st->sh.vad && !st->sh.vad_rows ? st->vbase.p : st->plan->base_rows.p; }

// Where a push delivers: rows (with decisions, if asked) or, on a set with signal state, samples; `capacity` and `counts` are of either
struct PushOutput {
    float *d_rows = nullptr;
    uint8_t *d_vad = nullptr;
    int16_t *d_sig = nullptr;
    int64_t capacity = 0;
    int64_t *counts = nullptr;
};

// Between stitch and carry on a set with rows out: the run, then the detector's, the trap's or the row kernels behind it
int push_rows(ctu_streams *st, int k, int n, const PushLayout &L, const RunExtent &x, const PushOutput &o, hipStream_t s) {
    const bool held = st->sh.g.held;
    const int rc = run_chain(st->eng, st->plan.get(), x, st->arena.p, held ? held_base(st) : o.d_rows, nullptr, s, !held, !st->sh.vad);
    if (rc != CTU_OK) return rc;
    if (st->sh.vad_rows) launch_stream_vad_rows(st, k, n, L, o.d_rows, o.d_vad, s);
    else if (st->sh.vad) launch_stream_vad(st, k, n, L, o.d_rows, o.d_vad, s);
    else if (st->sh.trap) launch_stream_trap(st, k, n, o.d_rows, s);
    else if (held) launch_stream_rows(st, k, n, L.most, false, o.d_rows, s);
    return CTU_OK;
}
// ... on a set with signal state: the front end leaves the time-domain frames of the push in the plan's ybuf, a row per frame (its SY
// instantiations - behind hwss / fwss / 2fwss run_chain's one streamed pass from the streams' slots; on 1024 .. 4096-point frames bigsynth_kernel from bigfft_kernel's), and stream_ola_kernel adds
// them onto every stream's tail - stream_ola_big_kernel a tail of more than OLA_TAIL_MAX entries
int push_signal(ctu_streams *st, int k, int n, const PushLayout &L, const RunExtent &x, const PushOutput &o, hipStream_t s) {
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const ctu_plan *pl = st->plan.get();
    e->in_signal_call = true;
    const int rc = run_chain(e, pl, x, st->arena.p, nullptr, nullptr, s, true);
    e->in_signal_call = false;
    if (rc != CTU_OK) return rc;
    if (e->tab.big) launch_bigsynth(e, pl, x, s, 1.0f / (float)d.wfft);  // (large transforms: bigfft_kernel exported the spectra)
    if (st->sh.ola_big) {  // the owner of every tail, then the slices of the samples past it
        const int64_t past = std::max<int64_t>(L.most - (d.window - d.wshift), 0);
        hipLaunchKernelGGL(stream_ola_big_kernel, dim3((unsigned)n, 1u + (unsigned)((past + OLA_SLICE - 1) / OLA_SLICE)), dim3(256), 0, s,
                           signal_params(st, st->sdesc.d[k].p, o.d_sig));
    } else {
        const unsigned slices = (unsigned)((L.most + OLA_SLICE - 1) / OLA_SLICE);
        hipLaunchKernelGGL(stream_ola_kernel, dim3((unsigned)n, slices), dim3(256), 0, s, signal_params(st, st->sdesc.d[k].p, o.d_sig));
    }
    HIP_TRY(hipGetLastError());
    return CTU_OK;
}

// How the new samples of a push lie in the caller's buffer: null layout - native int16_t, contiguous per stream, today's path; else the
// wire layout (checked by the caller: wire_layout_fault) and the element of it the buffer handed to the kernels starts at
struct PushSource {
    const ctu_wire_layout *wire = nullptr;
    int64_t base = 0;
};

// stream_stitch_wire_kernel by the layout: a contiguous source (stride 1) takes the instantiation with the wide loads
void launch_stitch_wire(const ctu_wire_layout &w, dim3 grid, hipStream_t s, const StreamParams &sp) {
    lift<CTU_WIRE_S16, CTU_WIRE_S16_SWAPPED, CTU_WIRE_ALAW, CTU_WIRE_MULAW>(w.format, [&](auto fmt) {
        lift<0, 1>(w.stride > 1 ? 1 : 0, [&](auto strided) {
            hipLaunchKernelGGL((stream_stitch_wire_kernel<decltype(fmt)::value, decltype(strided)::value != 0>), grid, dim3(256), 0, s, sp, (long long)w.stride);
        });
    });
}

// Every push: check, plan, commit, launch.  The set's kind says what goes out (rows: what of `o` is counted in rows; samples likewise)
int push_common(ctu_streams *st, bool want_signal, int32_t n, const int32_t *ids, const void *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                const PushOutput &o, void *stream, const PushSource &from = PushSource()) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const ctu_plan *pl = st->plan.get();
    const StreamSetShape &sh = st->sh;
    // ---- everything that can be refused is refused here or by the plan, ahead of the first launch and of any change to the set
    if (const char *m = wrong_call(st, want_signal, o.d_vad != nullptr, false)) return refuse(e, m);
    if (!push_args_ok(st, n, ids, n_samples)) return refuse(e, "push: bad stream count or null argument");
    if (n == 0) return CTU_OK;
    if (++st->push_no == 0) {  // (the counter wrapped: forget the marks)
        std::fill(st->seen.begin(), st->seen.end(), 0u);
        st->push_no = 1;
    }
    int64_t out = 0, fresh = 0;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= sh.n_streams) return refuse(e, "push: stream id out of range");
        if (st->seen[(size_t)ids[i]] == st->push_no) return refuse(e, "push: a stream id appears twice");
        st->seen[(size_t)ids[i]] = st->push_no;
        if (!push_count_ok(st, n_samples[i])) return refuse(e, "push: more samples than the set's max_push_samples (or fewer than none)");
        if (n_samples[i] && (!sample_off || sample_off[i] < 0)) return refuse(e, "push: null or negative sample offsets");
        const int64_t c = st->consumed[(size_t)ids[i]];
        out += sh.delivered(c + n_samples[i]) - sh.delivered(c);
        fresh += n_samples[i];
    }
    if (fresh && !d_pcm) return refuse(e, "push: null sample buffer");
    const char *const no_room = sh.signal ? "push: the samples of this push do not fit out_capacity" : "push: the rows of this push do not fit rows_capacity";
    // (samples are counted against the capacity by the plan, which lays them out anyway)
    if (sh.signal ? (o.capacity < 0 || (out && !o.d_sig)) : (out > o.capacity || (out && !o.d_rows))) return refuse(e, no_room);
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const int k = st->turn;
        HIP_TRY(hipEventSynchronize(st->desc_free[k]));  // (the push before last has read them; immediate before the first record)
        // ---- plan: the whole push, into this turn's page-locked descriptors and the set's scratch; the set itself is only read
        PushLayout L;
        L.push = st->desc.h[k]; L.rows = st->rdesc.h[k]; L.sig = st->sdesc.h[k]; L.heads = st->heads.h[k]; L.tail = st->chain_tail.data();
        L.row_counts = o.counts ? o.counts : st->counts.data();  // (the caller's array is output of the call: planned in place)
        L.consumed = st->next_consumed.data(); L.hsel = st->next_hsel.data(); L.replay = st->replay.h[k];
        if (sh.signal) L.capacity = o.capacity;
        if (sh.vad_rows) L.calls = st->vcalls.h[k];
        if (!stream_plan_push(sh.g, st->consumed.data(), st->hsel.data(), n, ids, n_samples, sample_off, L, from.base)) {
            if (L.over_capacity) return refuse(e, no_room);
            throw std::runtime_error("internal: a push beyond the set's arena");
        }
        // ---- commit: nothing refuses this push any more.  The mirrors take their next values; what follows is HIP calls alone
        st->turn ^= 1;
        for (int i = 0; i < n; i++) st->consumed[(size_t)ids[i]] = L.consumed[i];
        if (sh.g.held)
            for (int i = 0; i < n; i++) st->hsel[(size_t)ids[i]] = L.hsel[i];
        // ---- launch
        st->desc.upload(k, (size_t)n, s);
        if (sh.signal) st->sdesc.upload(k, (size_t)n, s);
        RunExtent x;  // the front end and its tails run over the front of the set's plan: this push
        x.n_tiles = L.tiles; x.grid = L.grid; x.total_frames = L.base_rows;
        x.heads = L.n_heads ? st->heads.d[k].p : pl->ext.heads;
        x.n_heads = L.n_heads ? L.n_heads : pl->ext.n_heads;
        x.xstate = st->xstate.p;
        StreamParams sp;
        sp.push = st->desc.d[k].p; sp.state = st->state.p; sp.carry = st->carry.p; sp.arena = st->arena.p; sp.src = static_cast<const int16_t *>(d_pcm); sp.tiles = pl->tiles.p;
        sp.cstride = sh.cstride; sp.window = d.window; sp.wshift = d.wshift;
        sp.n_tiles = L.tiles; sp.grid = L.grid;
        sp.tile_stream = L.n_heads ? pl->tile_utt.p : nullptr;
        if (L.n_heads) st->heads.upload(k, (size_t)L.n_heads, s);
        HIP_TRY(hipEventRecord(st->ev[0], s));
        if (from.wire) launch_stitch_wire(*from.wire, dim3((unsigned)n, (unsigned)L.slices), s, sp);
        else hipLaunchKernelGGL(stream_stitch_kernel, dim3((unsigned)n, (unsigned)L.slices), dim3(256), 0, s, sp);
        HIP_TRY(hipEventRecord(st->ev[1], s));
        HIP_TRY(hipGetLastError());
        const int rc = !L.tiles ? CTU_OK : sh.signal ? push_signal(st, k, n, L, x, o, s) : push_rows(st, k, n, L, x, o, s);
        HIP_TRY(hipEventRecord(st->ev[2], s));
        hipLaunchKernelGGL(stream_carry_kernel, dim3((unsigned)n), dim3(256), 0, s, sp);
        if (sh.g.held && sh.C > 0 && L.tiles && rc == CTU_OK) {
            RowParams rp;
            std::memset(&rp, 0, sizeof rp);
            rp.push = st->rdesc.d[k].p; rp.fresh = held_base(st); rp.hist = st->hist.p;
            rp.n_streams = sh.n_streams; rp.C = sh.C; rp.Dbase = sh.hw;
            hipLaunchKernelGGL(stream_rows_carry_kernel, dim3((unsigned)n, (unsigned)((sh.C * sh.hw + 255) / 256)), dim3(256), 0, s, rp);
        }
        HIP_TRY(hipEventRecord(st->ev[3], s));
        HIP_TRY(hipEventRecord(st->desc_free[k], s));
        HIP_TRY(hipGetLastError());
        st->timed = true;
        return rc;
    });
}

// The staging area of the host forms (and the device rows or samples ahead of the download), allocated on first use: n_streams *
// max_push_samples int16_t, which the host wire forms use by bytes
void host_stage_alloc(ctu_streams *st) {
    if (st->h_stage) return;
    ctu_engine *e = st->eng;
    const size_t cap = (size_t)st->sh.n_streams * (size_t)st->max_push;
    st->h_stage = static_cast<int16_t *>(ctu_host_alloc(cap * sizeof(int16_t)));
    if (!st->h_stage) throw std::runtime_error("page-locked staging of a stream set");
    st->d_stage.alloc(cap);
    // (a stream delivers wshift samples per frame, and a push completes frames out of its own samples and fewer than `window` carried ones)
    if (st->sh.signal) st->d_sig.alloc((size_t)st->sh.n_streams * ((size_t)st->max_push + (size_t)e->design->window));
    // (a push that brings a stream's frame wmax + 2 also delivers the rows of the wmax + 1 frames before it)
    else st->d_rows.alloc((size_t)std::max<int64_t>(st->plan->hp.total_frames + (int64_t)st->sh.n_streams * (st->sh.g.wmax + 1), 1) * e->design->D);
}
// The staging half of the host form of a push: the arguments checked, the staging area (and the device rows or samples ahead of the
// download) allocated on first use, the samples copied and uploaded, st->offs filled
int host_stage(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples) {
    ctu_engine *e = st->eng;
    if (!push_args_ok(st, n, ids, n_samples) || (n && !h_pcm)) return refuse(e, "push: bad stream count or null argument");
    int64_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (!push_count_ok(st, n_samples[i]) || (n_samples[i] && !h_pcm[i]))
            return refuse(e, "push: more samples than the set's max_push_samples (or fewer than none), or a null sample buffer");
        fresh += n_samples[i];
    }
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        host_stage_alloc(st);
        int64_t at = 0;
        for (int i = 0; i < n; i++) {
            st->offs[(size_t)i] = at;
            if (n_samples[i]) std::memcpy(st->h_stage + at, h_pcm[i], (size_t)n_samples[i] * sizeof(int16_t));
            at += n_samples[i];
        }
        if (fresh) HIP_TRY(hipMemcpyAsync(st->d_stage.p, st->h_stage, (size_t)fresh * sizeof(int16_t), hipMemcpyHostToDevice, nullptr));
        return CTU_OK;
    });
}
// ... and its tail: the counts of the push summed (where the push planned them), that many units of `unit` bytes down - split: page-locked
// memory at the link rate, pageable through the runtime's staging (as run_host_ranges downloads) - with the decisions, if asked
int host_fetch(ctu_streams *st, int32_t n, const int64_t *counts, void *h_out, const void *d_out, size_t unit, bool split, uint8_t *h_vad) {
    return guarded(st->eng, [&]() -> int {
        if (!counts) counts = st->counts.data();
        int64_t total = 0;
        for (int i = 0; i < n; i++) total += counts[i];
        if (total) {
            if (!split || is_pinned(h_out)) HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)total * unit, hipMemcpyDeviceToHost, nullptr));
            else HIP_TRY(hipMemcpy(h_out, d_out, (size_t)total * unit, hipMemcpyDeviceToHost));
            if (h_vad) HIP_TRY(hipMemcpyAsync(h_vad, st->vsink.p, (size_t)total, hipMemcpyDeviceToHost, nullptr));
        }
        HIP_TRY(hipStreamSynchronize(nullptr));
        return CTU_OK;
    });
}
}  // namespace

int ctu_streams_push(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                     float *d_rows, int64_t rows_capacity, int64_t *row_counts, void *stream) {
    return ctu_streams_push_vad(st, n, ids, d_pcm, sample_off, n_samples, d_rows, rows_capacity, row_counts, nullptr, stream);
}

int ctu_streams_push_vad(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                         float *d_rows, int64_t rows_capacity, int64_t *row_counts, uint8_t *d_vad, void *stream) {
    PushOutput o;
    o.d_rows = d_rows; o.d_vad = d_vad; o.capacity = rows_capacity; o.counts = row_counts;
    return push_common(st, false, n, ids, d_pcm, sample_off, n_samples, o, stream);
}

int ctu_streams_push_signal(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                            int16_t *d_out, int64_t out_capacity, int64_t *out_counts, void *stream) {
    PushOutput o;
    o.d_sig = d_out; o.capacity = out_capacity; o.counts = out_counts;
    return push_common(st, true, n, ids, d_pcm, sample_off, n_samples, o, stream);
}

int ctu_streams_push_host(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples, float *h_rows,
                          int64_t rows_capacity, int64_t *row_counts) {
    return ctu_streams_push_vad_host(st, n, ids, h_pcm, n_samples, h_rows, rows_capacity, row_counts, nullptr);
}

int ctu_streams_push_vad_host(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples, float *h_rows,
                              int64_t rows_capacity, int64_t *row_counts, uint8_t *h_vad) {
    if (!st) return CTU_ERR_INPUT;
    if (const char *m = wrong_call(st, false, h_vad != nullptr, false)) return refuse(st->eng, m);
    if (const int rc = host_stage(st, n, ids, h_pcm, n_samples); rc != CTU_OK) return rc;
    // the device rows hold any push of the set; what the caller's buffer holds is the device form's check
    const int rc = ctu_streams_push_vad(st, n, ids, st->d_stage.p, st->offs.data(), n_samples, h_rows ? st->d_rows.p : nullptr, h_rows ? rows_capacity : 0,
                                        row_counts, h_vad ? st->vsink.p : nullptr, nullptr);
    if (rc != CTU_OK) return rc;
    return host_fetch(st, n, row_counts, h_rows, st->d_rows.p, (size_t)st->eng->design->D * 4, true, h_vad);
}

int ctu_streams_push_signal_host(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples, int16_t *h_out,
                                 int64_t out_capacity, int64_t *out_counts) {
    if (!st) return CTU_ERR_INPUT;
    if (const char *m = wrong_call(st, true, false, false)) return refuse(st->eng, m);
    if (const int rc = host_stage(st, n, ids, h_pcm, n_samples); rc != CTU_OK) return rc;
    // the device samples hold any push of the set; what the caller's buffer holds is the device form's check
    const int rc = ctu_streams_push_signal(st, n, ids, st->d_stage.p, st->offs.data(), n_samples, h_out ? st->d_sig.p : nullptr, h_out ? out_capacity : 0,
                                           out_counts, nullptr);
    if (rc != CTU_OK) return rc;
    return host_fetch(st, n, out_counts, h_out, st->d_sig.p, sizeof(int16_t), false, nullptr);
}

// ---- wire input: the pushes above with the samples read through a ctu_wire_layout (stream_stitch_wire_kernel expands them on their way
// into the slots; everything behind the stitch works from the push arena and is the plain push's)
namespace {
// The layout's own refusals, ahead of everything a push refuses
int wire_refusal(ctu_streams *st, const ctu_wire_layout *w, const void *buf) {
    if (const char *m = wire_layout_fault(w, buf)) return refuse(st->eng, std::string("push: ") + m);
    return CTU_OK;
}
// The staging half of the host wire forms: the arguments checked, the covering range of the push uploaded in one copy - from a
// page-locked buffer as it lies, from a pageable one through the set's page-locked staging - and its first element in *first
int host_stage_wire(ctu_streams *st, int32_t n, const int32_t *ids, const void *h_in, const int64_t *elem_off, const int64_t *n_samples,
                    const ctu_wire_layout *w, int64_t *first) {
    ctu_engine *e = st->eng;
    if (const int rc = wire_refusal(st, w, h_in); rc != CTU_OK) return rc;
    if (!push_args_ok(st, n, ids, n_samples)) return refuse(e, "push: bad stream count or null argument");
    int64_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (!push_count_ok(st, n_samples[i])) return refuse(e, "push: more samples than the set's max_push_samples (or fewer than none)");
        if (n_samples[i] && (!elem_off || elem_off[i] < 0)) return refuse(e, "push: null or negative element offsets");
        fresh += n_samples[i];
    }
    if (fresh && !h_in) return refuse(e, "push: null sample buffer");
    const int64_t extent = wire_extent(w, n, elem_off, n_samples, first);
    const size_t cap = (size_t)st->sh.n_streams * (size_t)st->max_push;
    if (extent < 0 || (uint64_t)extent > cap)
        return refuse(e, "push: the covering range of a host wire push is more than n_streams * max_push_samples elements (a sparse layout: the "
                         "device form or the per-pointer calls)");
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        host_stage_alloc(st);
        if (extent) {
            const size_t unit = (size_t)wire_elem_bytes(w->format), bytes = (size_t)extent * unit;
            const uint8_t *src = static_cast<const uint8_t *>(h_in) + (size_t)*first * unit;
            if (!is_pinned(src)) {
                std::memcpy(st->h_stage, src, bytes);
                src = reinterpret_cast<const uint8_t *>(st->h_stage);
            }
            HIP_TRY(hipMemcpyAsync(st->d_stage.p, src, bytes, hipMemcpyHostToDevice, nullptr));
        }
        return CTU_OK;
    });
}
// (the upload may still read the caller's buffer when the device form refuses: a host form is synchronised on return)
int host_wire_done(int rc) {
    if (rc != CTU_OK) (void)hipStreamSynchronize(nullptr);
    return rc;
}
}  // namespace

int ctu_streams_push_wire(ctu_streams *st, int32_t n, const int32_t *ids, const void *d_in, const int64_t *elem_off, const int64_t *n_samples,
                          const ctu_wire_layout *w, float *d_rows, int64_t rows_capacity, int64_t *row_counts, uint8_t *d_vad, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    if (const int rc = wire_refusal(st, w, d_in); rc != CTU_OK) return rc;
    PushOutput o;
    o.d_rows = d_rows; o.d_vad = d_vad; o.capacity = rows_capacity; o.counts = row_counts;
    PushSource from;
    from.wire = w;
    return push_common(st, false, n, ids, d_in, elem_off, n_samples, o, stream, from);
}

int ctu_streams_push_signal_wire(ctu_streams *st, int32_t n, const int32_t *ids, const void *d_in, const int64_t *elem_off, const int64_t *n_samples,
                                 const ctu_wire_layout *w, int16_t *d_out, int64_t out_capacity, int64_t *out_counts, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    if (const int rc = wire_refusal(st, w, d_in); rc != CTU_OK) return rc;
    PushOutput o;
    o.d_sig = d_out; o.capacity = out_capacity; o.counts = out_counts;
    PushSource from;
    from.wire = w;
    return push_common(st, true, n, ids, d_in, elem_off, n_samples, o, stream, from);
}

int ctu_streams_push_wire_host(ctu_streams *st, int32_t n, const int32_t *ids, const void *h_in, const int64_t *elem_off, const int64_t *n_samples,
                               const ctu_wire_layout *w, float *h_rows, int64_t rows_capacity, int64_t *row_counts, uint8_t *h_vad) {
    if (!st) return CTU_ERR_INPUT;
    if (const char *m = wrong_call(st, false, h_vad != nullptr, false)) return refuse(st->eng, m);
    PushSource from;
    from.wire = w;
    if (const int rc = host_stage_wire(st, n, ids, h_in, elem_off, n_samples, w, &from.base); rc != CTU_OK) return rc;
    PushOutput o;  // the device rows hold any push of the set; what the caller's buffer holds is the device form's check
    o.d_rows = h_rows ? st->d_rows.p : nullptr; o.d_vad = h_vad ? st->vsink.p : nullptr; o.capacity = h_rows ? rows_capacity : 0; o.counts = row_counts;
    if (const int rc = host_wire_done(push_common(st, false, n, ids, st->d_stage.p, elem_off, n_samples, o, nullptr, from)); rc != CTU_OK) return rc;
    return host_fetch(st, n, row_counts, h_rows, st->d_rows.p, (size_t)st->eng->design->D * 4, true, h_vad);
}

int ctu_streams_push_signal_wire_host(ctu_streams *st, int32_t n, const int32_t *ids, const void *h_in, const int64_t *elem_off, const int64_t *n_samples,
                                      const ctu_wire_layout *w, int16_t *h_out, int64_t out_capacity, int64_t *out_counts) {
    if (!st) return CTU_ERR_INPUT;
    if (const char *m = wrong_call(st, true, false, false)) return refuse(st->eng, m);
    PushSource from;
    from.wire = w;
    if (const int rc = host_stage_wire(st, n, ids, h_in, elem_off, n_samples, w, &from.base); rc != CTU_OK) return rc;
    PushOutput o;  // the device samples hold any push of the set; what the caller's buffer holds is the device form's check
    o.d_sig = h_out ? st->d_sig.p : nullptr; o.capacity = h_out ? out_capacity : 0; o.counts = out_counts;
    if (const int rc = host_wire_done(push_common(st, true, n, ids, st->d_stage.p, elem_off, n_samples, o, nullptr, from)); rc != CTU_OK) return rc;
    return host_fetch(st, n, out_counts, h_out, st->d_sig.p, sizeof(int16_t), false, nullptr);
}

int64_t ctu_wire_extent(const ctu_wire_layout *w, int32_t n, const int64_t *elem_off, const int64_t *n_samples, int64_t *first) {
    return wire_extent(w, n, elem_off, n_samples, first);
}

int64_t ctu_wire_expand(const ctu_wire_layout *w, const void *in, int64_t elem_off, int64_t n_samples, int16_t *out) {
    return wire_expand(w, in, elem_off, n_samples, out);
}

int ctu_streams_finish(ctu_streams *st, int32_t id, float *d_rows, int64_t rows_capacity, int64_t *row_count, void *stream) {
    return ctu_streams_finish_vad(st, id, d_rows, rows_capacity, row_count, nullptr, stream);
}

int ctu_streams_finish_vad(ctu_streams *st, int32_t id, float *d_rows, int64_t rows_capacity, int64_t *row_count, uint8_t *d_vad, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const StreamSetShape &sh = st->sh;
    if (const char *m = wrong_call(st, false, d_vad != nullptr, true)) return refuse(e, m);
    if (id < 0 || id >= sh.n_streams) return refuse(e, "finish: stream id out of range");
    if (row_count) *row_count = 0;  // fread() comes up short on a trailing partial window and the file ends there (src/io/in.cc:314,438)
    const int64_t total = st->consumed[(size_t)id];
    const FinishLayout fin = stream_plan_finish(d.window, d.wshift, sh.g.H, sh.g.wmax, total, id, st->hsel[(size_t)id], sh.vad && !sh.vad_rows, false, sh.g.vh);
    const int64_t pending = fin.pending;
    const bool too_short = fin.too_short;
    // ahead of any launch or change: the stream stays as it was
    if (pending > rows_capacity || (pending && !d_rows)) return refuse(e, "finish: the rows held back for this stream do not fit rows_capacity");
    st->consumed[(size_t)id] = 0;
    hipStream_t s = (hipStream_t)stream;
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        if (pending) {  // rows r0 .. F - 1 with the file's length known: every base row they read is in the history
            const int k = st->turn;
            st->turn ^= 1;
            HIP_TRY(hipEventSynchronize(st->desc_free[k]));
            st->rdesc.h[k][0] = fin.row;
            if (sh.vad_rows) {  // the calls the file still owes and the filter's flush, then the rows with the file's length known
                launch_stream_rows(st, k, 1, pending, true, d_rows, s);
                if (d_vad) {
                    StreamVadParams vp;
                    std::memset(&vp, 0, sizeof vp);
                    vp.push = st->rdesc.d[k].p; vp.vstate = st->vstate.p; vp.vad = d_vad;
                    hipLaunchKernelGGL(stream_vad_delayed_finish_kernel, dim3(1), dim3(64), 0, s, vp, e->vp, stream_vad_delay(st, nullptr), fin.calls);
                    HIP_TRY(hipGetLastError());
                }
            } else if (sh.vad) {  // the filter's flush and the h rows it releases, with the file's length known
                st->rdesc.upload(k, 1, s);
                RowParams rp;
                std::memset(&rp, 0, sizeof rp);
                rp.push = st->rdesc.d[k].p; rp.hist = st->hist.p; rp.rows = d_rows;
                rp.n_streams = sh.n_streams; rp.C = sh.C; rp.Dbase = d.Dbase; rp.finishing = 1;
                hipLaunchKernelGGL(stream_vad_finish_kernel, dim3(1), dim3(256), 0, s, rp, d.D, st->vstate.p, d_vad, d.o.vad_filter_order);
                HIP_TRY(hipGetLastError());
            } else if (sh.trap) launch_stream_trap(st, k, 1, d_rows, s);  // (Tn = 0: the newest frame is the file's last)
            else launch_stream_rows(st, k, 1, pending, true, d_rows, s);
            HIP_TRY(hipEventRecord(st->desc_free[k], s));
        }
        HIP_TRY(hipMemsetAsync(st->state.p + id, 0, sizeof(StreamState), s));
        if (sh.g.held && (!sh.vad || sh.vad_rows)) HIP_TRY(hipMemsetAsync(st->means.p + (size_t)id * STREAM_MEANS, 0, STREAM_MEANS * sizeof(float), s));
        if (sh.trap)  // both histories of the stream (a new file reads neither ahead of its own rows: the left clamp is frame 0)
            for (int h = 0; h < 2; h++)
                HIP_TRY(hipMemsetAsync(st->hist.p + ((size_t)h * sh.n_streams + id) * sh.C * sh.hw, 0, (size_t)sh.C * sh.hw * sizeof(float), s));
        return CTU_OK;
    });
    if (rc != CTU_OK) return rc;
    if (total > 0 && total < d.window - d.wshift) {
        set_error(e, "IO: Signal shorter than one frame!");  // src/io/in.cc:277; the stream is reset all the same
        return CTU_ERR_INPUT;
    }
    // the words of an offline plan's refusals (plan.cc); the stream is reset all the same
    if (too_short && sh.trap) return refuse(e, "trapdct on fewer than (traplen+1)/2 frames is undefined in the reference (src/fea/fea_trap.cc:64-70)");
    if (too_short) return refuse(e, "delta / stacking on fewer than window+2 frames is ill-defined in the reference (src/fea/fea_delta.cc:74-130,178-206)");
    if (row_count) *row_count = pending;
    return CTU_OK;
}

int ctu_streams_finish_host(ctu_streams *st, int32_t id, float *h_rows, int64_t rows_capacity, int64_t *row_count) {
    return ctu_streams_finish_vad_host(st, id, h_rows, rows_capacity, row_count, nullptr);
}

int ctu_streams_finish_vad_host(ctu_streams *st, int32_t id, float *h_rows, int64_t rows_capacity, int64_t *row_count, uint8_t *h_vad) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    if (const char *m = wrong_call(st, false, h_vad != nullptr, true)) return refuse(e, m);
    const int D = e->design->D;
    if (row_count) *row_count = 0;
    const int64_t pending = ctu_streams_pending(st, id);  // (at most max(H, wmax + 1) rows; an id outside the set is ctu_streams_finish's to refuse)
    DevBuf<float> rows;
    int64_t cnt = 0;
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        if (pending > 0) rows.alloc((size_t)pending * D);
        const int rc = ctu_streams_finish_vad(st, id, h_rows ? rows.p : nullptr, h_rows ? rows_capacity : 0, &cnt, h_vad ? st->vsink.p : nullptr, nullptr);
        if (rc != CTU_OK) return rc;
        if (cnt) HIP_TRY(hipMemcpy(h_rows, rows.p, (size_t)cnt * D * 4, hipMemcpyDeviceToHost));
        if (cnt && h_vad) HIP_TRY(hipMemcpy(h_vad, st->vsink.p, (size_t)cnt, hipMemcpyDeviceToHost));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return CTU_OK;
    });
    if (rc == CTU_OK && row_count) *row_count = cnt;
    return rc;
}

int ctu_streams_finish_signal(ctu_streams *st, int32_t id, int16_t *d_out, int64_t out_capacity, int64_t *out_count, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    if (const char *m = wrong_call(st, true, false, true)) return refuse(e, m);
    if (id < 0 || id >= st->sh.n_streams) return refuse(e, "finish: stream id out of range");
    if (out_count) *out_count = 0;
    const int64_t total = st->consumed[(size_t)id];
    const FinishLayout fin = stream_plan_finish(d.window, d.wshift, 0, 0, total, id, 0, false, true);
    // ahead of any launch or change: the stream stays as it was
    if (fin.pending > out_capacity || (fin.pending && !d_out)) return refuse(e, "finish: the samples of this stream's tail do not fit out_capacity");
    st->consumed[(size_t)id] = 0;
    hipStream_t s = (hipStream_t)stream;
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        // the tail rounded and cleared (a file without a frame has added nothing to it); the noise estimate needs no clearing: the first
        // tile of a file starts from the reference's initial one (frontend_kernel: rec.t0 == 0), as behind ctu_streams_finish
        if (fin.pending) hipLaunchKernelGGL(stream_ola_flush_kernel, dim3(1), dim3(256), 0, s, signal_params(st, nullptr, d_out), fin.sig);
        HIP_TRY(hipMemsetAsync(st->state.p + id, 0, sizeof(StreamState), s));
        HIP_TRY(hipGetLastError());
        return CTU_OK;
    });
    if (rc != CTU_OK) return rc;
    if (total > 0 && total < d.window - d.wshift) {
        set_error(e, "IO: Signal shorter than one frame!");  // src/io/in.cc:277; the stream is reset all the same
        return CTU_ERR_INPUT;
    }
    if (out_count) *out_count = fin.pending;
    return CTU_OK;
}

int ctu_streams_finish_signal_host(ctu_streams *st, int32_t id, int16_t *h_out, int64_t out_capacity, int64_t *out_count) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    if (const char *m = wrong_call(st, true, false, true)) return refuse(e, m);
    if (out_count) *out_count = 0;
    const int64_t pending = ctu_streams_pending(st, id);  // (an id outside the set is ctu_streams_finish_signal's to refuse)
    DevBuf<int16_t> out;
    int64_t cnt = 0;
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        if (pending > 0) out.alloc((size_t)pending);
        const int rc = ctu_streams_finish_signal(st, id, h_out ? out.p : nullptr, h_out ? out_capacity : 0, &cnt, nullptr);
        if (rc != CTU_OK) return rc;
        if (cnt) HIP_TRY(hipMemcpy(h_out, out.p, (size_t)cnt * sizeof(int16_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return CTU_OK;
    });
    if (rc == CTU_OK && out_count) *out_count = cnt;
    return rc;
}

int ctu_streams_last_push_ms(ctu_streams *st, float *ms3) {
    if (!st || !ms3 || !st->timed) return CTU_ERR_INPUT;
    if (hipEventSynchronize(st->ev[3]) != hipSuccess) return CTU_ERR_DEVICE;
    if (hipEventElapsedTime(&ms3[0], st->ev[0], st->ev[1]) != hipSuccess) return CTU_ERR_DEVICE;
    if (hipEventElapsedTime(&ms3[1], st->ev[1], st->ev[2]) != hipSuccess) return CTU_ERR_DEVICE;
    if (hipEventElapsedTime(&ms3[2], st->ev[2], st->ev[3]) != hipSuccess) return CTU_ERR_DEVICE;
    return CTU_OK;
}
