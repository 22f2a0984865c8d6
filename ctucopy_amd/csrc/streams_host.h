// Streaming input (include/ctu_engine.h: ctu_streams_*), host side: the stream set, its creation, pushes and finishes.
// Included by engine.hip inside its extern "C" block, behind everything a run is made of (one translation unit).
//
// A push is check, plan, commit, launch.  The checks refuse ahead of everything else.  stream_plan_push (stream_plan.h, host only, also
// compiled and tested without HIP) then lays the whole push out from the set's mirrors without touching them.  The commit copies the
// mirrors' next values into the set, and from there on a push is HIP calls alone, sized by the plan (two HIP calls come ahead of the
// plan: the device is selected, and the plan waits for this turn's page-locked descriptors, which it writes, to be free): the run goes over the front of the
// set's ctu_plan with the extent of the push (RunExtent), so the plan itself is not written after ctu_streams_create_ex.
// On a set with detector state the run stops ahead of the VAD's sequential stages (run_chain: vad_stages off) and launch_stream_vad
// replays them from the set's own state, by the plan's RowPush descriptors and its list of the streams that complete a frame.
// On a set with signal state (speech output) the run leaves the time-domain frames of the push in the plan's ybuf and stream_ola_kernel
// adds them onto every stream's tail of the overlap-add (stream_signal_kernels.h): ctu_streams_push_signal / ctu_streams_finish_signal.
// A HIP call that fails behind the commit (CTU_ERR_DEVICE) leaves mirrors and device state out of step: include/ctu_engine.h says what
// the caller may still do with the set.
#pragma once

// A stream set (ctu_streams_create): per-stream state in HBM, and what a push needs that does not change from push to push - a plan over
// n_streams utterances of the longest stitched length (its HostPlan, plan_host.h, is where the set reads the arena size, the tile and row
// totals from), whose tile list, chain heads (workgroup g starts at tile g), arena and scratch a push uses the front of.  The tile records themselves are written by stream_stitch_kernel, push after push.
struct ctu_streams {
    ctu_engine *eng = nullptr;
    int n_streams = 0, cstride = 0;
    int64_t max_push = 0;
    PushGeom g{};                    // what stream_plan_push lays a push out by: window and hop, halo, row / noise state, chain and arena limits
    std::unique_ptr<const ctu_plan> plan;  // (const: a push runs the front of it by a RunExtent of its own, nothing writes it after create)
    DevBuf<int16_t> arena, carry;
    DevBuf<StreamState> state;
    std::vector<int64_t> consumed;   // the host's mirror of StreamState::consumed: layout and row counts of a push need no copy back
    std::vector<int64_t> next_consumed;  // (of the push at hand, by position in it: PushLayout::consumed)
    std::vector<int64_t> counts;         // (PushLayout::row_counts of a push whose caller passes no array; the host form reads them here)
    std::vector<uint32_t> seen;      // the push a stream was last named in (a repeat inside one push is refused)
    uint32_t push_no = 0;
    // the descriptors of a push: two page-locked buffers and their device copies in turn, each guarded by the event behind its last reader
    StreamPush *h_desc[2] = {nullptr, nullptr};
    DevBuf<StreamPush> d_desc[2];
    hipEvent_t desc_free[2] = {nullptr, nullptr};
    int turn = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around stream_stitch_kernel and stream_carry_kernel of the last push
    bool timed = false;
    // CTU_STREAMS_ROW_STATE with a delta chain, stacking or CMS (stream_rows_kernels.h; g.held, g.H, g.wmax): the history's rows, the two
    // histories of every stream and which one is current, the running means, the descriptors of the row kernels
    int C = 0;
    DevBuf<float> hist, means;
    std::vector<uint8_t> hsel, next_hsel;
    RowPush *h_rdesc[2] = {nullptr, nullptr};
    DevBuf<RowPush> d_rdesc[2];
    // CTU_STREAMS_NR_STATE on a chain with -nr_mode exten (g.chained, g.max_chains): Navg | Yavg of every stream (frontend_kernel<..., XS>;
    // with CTU_STREAMS_LARGE_STATE on 1024 .. 4096 points wave1k_kernel<true, XS> / bigfft_kernel<NIT, true, XS>: sized by the kernel that runs),
    // the heads of the chains a push is dealt onto, which travel as the descriptors do, and the stream of every tile.
    // CTU_STREAMS_SS_STATE on a chain with -nr_mode hwss | fwss | 2fwss: the same buffer and the same chains, a slot of xs_ss_floats
    // (layout_constants.h) per stream - Navg | Nravg and the detector's record (frontend_kernel<..., SS, ..., XS>)
    DevBuf<float> xstate;
    int *h_heads[2] = {nullptr, nullptr};
    DevBuf<int> d_heads[2];
    std::vector<int> chain_tail;     // (scratch of stream_plan_push)
    // CTU_STREAMS_VAD_STATE on a configuration with the VAD module (stream_vad_kernels.h; g.vad, g.H = h, g.wmax = h - 1): the detector's
    // record of every stream, the base rows of a push ahead of their delayed copy (h > 0: the histories above hold the last h of them),
    // the decisions of a push nobody asked for (and of the host forms, ahead of the download), the streams of a push that run the replay
    bool vad = false;
    DevBuf<double> vstate;
    DevBuf<float> vbase;
    DevBuf<uint8_t> vsink;
    int *h_replay[2] = {nullptr, nullptr};
    DevBuf<int> d_replay[2];
    // CTU_STREAMS_SIGNAL_STATE on a configuration with speech output (stream_signal_kernels.h; g.signal): the overlap-add's tail of every
    // stream - tstride doubles each, window - wshift of them in use - and the descriptors of stream_ola_kernel; ola_big: a tail beyond
    // OLA_TAIL_MAX entries (CTU_STREAMS_LARGE_STATE), which stream_ola_big_kernel carries
    bool signal = false, ola_big = false;
    int tstride = 0;
    DevBuf<double> otail;
    SignalPush *h_sdesc[2] = {nullptr, nullptr};
    DevBuf<SignalPush> d_sdesc[2];
    // CTU_STREAMS_TRAP_STATE on a configuration with -fea_kind trapdct (stream_trap_kernels.h; g.held, g.H = half, g.wmax = half - 1):
    // the histories above hold the last C = 2 half log-mel rows of every stream, hw = B floats each; the stream of every column of
    // stream_trap_kernel, which travels as the descriptors do
    bool trap = false;
    int hw = 0;                      // floats of a history row: Dbase, or B with trap state
    int *h_cols[2] = {nullptr, nullptr};
    DevBuf<int> d_cols[2];
    // the host form: page-locked staging of the new samples, their device copy, the rows (the samples) ahead of the download
    int16_t *h_stage = nullptr;
    DevBuf<int16_t> d_stage;
    DevBuf<float> d_rows;
    DevBuf<int16_t> d_sig;
    std::vector<int64_t> offs;
    ~ctu_streams() {
        for (StreamPush *h : h_desc) ctu_host_free(h);
        for (RowPush *h : h_rdesc) ctu_host_free(h);
        for (SignalPush *h : h_sdesc) ctu_host_free(h);
        for (int *h : h_heads) ctu_host_free(h);
        for (int *h : h_replay) ctu_host_free(h);
        for (int *h : h_cols) ctu_host_free(h);
        ctu_host_free(h_stage);
        for (hipEvent_t v : desc_free)
            if (v) (void)hipEventDestroy(v);
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
    }
};

namespace {
void design_halo(const ctu::Design &d, int *H, int *wmax) { stream_halo(d.post_order, d.post_w, d.post_stack, H, wmax); }
int64_t stream_rows_of(const ctu_streams *st, int64_t F) { return stream_rows_out(st->g.H, st->g.wmax, F); }
// a set with detector state on a configuration with the VAD module: the majority filter's delay is the halo (nothing else holds rows there)
bool streams_vad(const ctu::Design &d, uint32_t flags) { return (flags & CTU_STREAMS_VAD_STATE) && d.o.do_vad(); }
// a set with signal state on a configuration with speech output: samples go out, by the *_signal calls
bool streams_signal(const ctu::Design &d, uint32_t flags) { return (flags & CTU_STREAMS_SIGNAL_STATE) && d.signal_out; }
// the samples the finish of a stream with F frames delivers: the overlap-add's tail, once there is a frame
int64_t signal_pending(const ctu::Design &d, int64_t F) { return F > 0 ? d.window - d.wshift : 0; }
// a set with trap state on a configuration with -fea_kind trapdct: half a context is the halo (nothing else holds rows there: delta
// chains, stacking and CMS are refused on trapdct at create)
bool streams_trap(const ctu::Design &d, uint32_t flags) { return (flags & CTU_STREAMS_TRAP_STATE) && d.kind == ctu::FeaKind::TrapDct; }
}  // namespace

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
        design_halo(d, &H, &wmax);
        if (streams_vad(d, flags)) stream_vad_halo(d.o.vad_filter_order, &H, &wmax);
        if (streams_trap(d, flags)) stream_trap_halo(d.o.fea_trapdct_traplen, &H, &wmax);
        if (halo) *halo = H;
        return CTU_OK;
    } catch (const std::exception &ex) {
        say(ex.what());
        return CTU_ERR_OPTS;
    }
}

int64_t ctu_streams_step(int32_t window, int32_t wshift, int64_t total, int64_t *carry) {
    if (window < 1 || wshift < 1 || wshift > window || total < 0) return CTU_ERR_INPUT;
    const int64_t F = stream_frames(total, window, wshift);
    if (carry) *carry = total - F * wshift;
    return F;
}

int64_t ctu_streams_rows_step(int32_t window, int32_t wshift, int32_t halo, int32_t wmax, int64_t total, int64_t *pending) {
    // (a chain's largest window is at least 1; trapdct's rule is wmax = halo - 1, which is 0 for a context of three frames)
    if (window < 1 || wshift < 1 || wshift > window || total < 0 || halo < 0 || wmax < 0 || wmax > halo || (halo > 0 && wmax < 1 && wmax != halo - 1)) return CTU_ERR_INPUT;
    const int64_t F = stream_frames(total, window, wshift), R = stream_rows_out(halo, wmax, F);
    if (pending) *pending = F - R;
    return R;
}

int64_t ctu_streams_vad_step(int32_t window, int32_t wshift, int32_t filter_order, int64_t total, int64_t *pending) {
    if (window < 1 || wshift < 1 || wshift > window || total < 0 || filter_order < 1 || filter_order > 31) return CTU_ERR_INPUT;
    int H = 0, wmax = 0;
    stream_vad_halo(filter_order, &H, &wmax);
    const int64_t F = stream_frames(total, window, wshift), R = stream_rows_out(H, wmax, F);
    if (pending) *pending = F - R;
    return R;
}

int ctu_streams_create(ctu_engine *e, int32_t n_streams, int64_t max_push_samples, ctu_streams **out) {
    return ctu_streams_create_ex(e, n_streams, max_push_samples, 0, out);
}

int ctu_streams_create_ex(ctu_engine *e, int32_t n_streams, int64_t max_push_samples, uint32_t flags, ctu_streams **out) {
    if (!e || !out) return CTU_ERR_INPUT;
    *out = nullptr;
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
    // (per-wave chains are exten's with the noise state, or those of hwss / fwss / 2fwss with the subtraction state, on the 256- / 512-point front end)
    const bool ss_set = e->tab.ss && (flags & CTU_STREAMS_SS_STATE) && !e->tab.big && !e->tab.ss_file && !d.signal_out;
    if ((e->geom.per_wave && !e->tab.ss && !(flags & CTU_STREAMS_NR_STATE)) || (e->geom.do_vad && !(flags & CTU_STREAMS_VAD_STATE)) || (e->tab.ss && !ss_set) || (e->geom.per_wave && e->tab.big && !(flags & CTU_STREAMS_LARGE_STATE)) || (e->geom.do_vad && e->tab.big)) {
        set_error(e, "ENGINE: internal: a streamed configuration with chains of whole utterances");
        return CTU_ERR_UNSUPPORTED;
    }
    std::unique_ptr<ctu_streams> st(new ctu_streams);
    st->eng = e;
    st->n_streams = n_streams;
    st->max_push = max_push_samples;
    st->cstride = (d.window + 7) / 8 * 8;
    PushGeom &g = st->g;
    g.window = d.window;
    g.wshift = d.wshift;
    g.max_wg = e->geom.max_wg;
    g.held = d.post_order > 0 || d.cms;  // (only with CTU_STREAMS_ROW_STATE: refused above without)
    design_halo(d, &g.H, &g.wmax);
    st->vad = g.vad = streams_vad(d, flags);
    if (st->vad) {  // (no chain, no CMS beside the detector: refused above) the filter's delay holds the rows back
        stream_vad_halo(d.o.vad_filter_order, &g.H, &g.wmax);
        g.held = g.H > 0;
    }
    st->trap = streams_trap(d, flags);
    if (st->trap) {  // (no chain, no CMS, no detector beside trapdct: refused above) half a context holds the rows back
        stream_trap_halo(d.o.fea_trapdct_traplen, &g.H, &g.wmax);
        g.held = true;
    }
    st->signal = g.signal = streams_signal(d, flags);
    if (st->signal) {  // (speech output writes no rows: whatever the command line says of a delta chain or CMS, nothing is held)
        g.held = false;
        g.H = g.wmax = 0;
        st->tstride = (std::max(d.window - d.wshift, 1) + 1) / 2 * 2;
        st->ola_big = d.window - d.wshift > OLA_TAIL_MAX;
        if (((st->ola_big || e->tab.big) && !(flags & CTU_STREAMS_LARGE_STATE)) || d.window - d.wshift > OLA_BIG_TAIL_MAX) {
            set_error(e, "ENGINE: internal: a signal set beyond the 512-point front end");
            return CTU_ERR_UNSUPPORTED;
        }
    }
    g.chained = e->geom.per_wave;  // (exten with CTU_STREAMS_NR_STATE, hwss / fwss / 2fwss with CTU_STREAMS_SS_STATE: everything else with chains of whole files is refused above)
    g.max_chains = e->geom.chain_slots;  // (the plan geometry's: max_wg * NWAVE wave chains, or n_cu * 8 workgroup chains of bigfft_kernel)
    st->hw = st->trap ? d.B : d.Dbase;
    st->C = st->vad ? g.H : st->trap ? 2 * g.H : g.held ? std::max(2 * g.H, g.H + (d.cms == 2 ? d.o.length_b : 1) - 1) : 0;  // (detector state: a row is copied h frames late, nothing more)
    st->consumed.assign((size_t)n_streams, 0);
    st->seen.assign((size_t)n_streams, 0);
    st->hsel.assign((size_t)n_streams, 0);
    st->offs.assign((size_t)n_streams, 0);
    // what a planned push is written into: a push allocates nothing
    st->next_consumed.assign((size_t)n_streams, 0);
    st->counts.assign((size_t)n_streams, 0);
    st->next_hsel.assign((size_t)n_streams, 0);
    const size_t n_heads = (size_t)chain_deal(n_streams, g.max_chains).heads();
    if (g.chained) st->chain_tail.assign(n_heads, -1);
    // the longest slot: the lead, a full carry, a full push (and no shorter than the shortest file a delta chain is defined on: the plan
    // of a set whose pushes are shorter than that is still a plan of files that could be)
    const std::vector<int64_t> longest((size_t)n_streams, std::max((int64_t)STREAM_LEAD + d.window - 1 + max_push_samples,
                                                                   (int64_t)d.window + (int64_t)(g.wmax + 1) * d.wshift));
    ctu_plan *pl = nullptr;
    if (const int rc = ctu_plan_create(e, longest.data(), n_streams, &pl); rc != CTU_OK) return rc;
    st->plan.reset(pl);
    g.arena_samples = pl->hp.total_samples;
    g.tile_cap = (int64_t)pl->hp.tiles.size();
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        st->arena.alloc((size_t)pl->hp.total_samples);
        st->carry.alloc((size_t)n_streams * st->cstride);
        st->state.alloc((size_t)n_streams);
        HIP_TRY(hipMemset(st->arena.p, 0, st->arena.n * sizeof(int16_t)));
        HIP_TRY(hipMemset(st->carry.p, 0, st->carry.n * sizeof(int16_t)));
        HIP_TRY(hipMemset(st->state.p, 0, st->state.n * sizeof(StreamState)));
        for (int k = 0; k < 2; k++) {
            st->h_desc[k] = static_cast<StreamPush *>(ctu_host_alloc((size_t)n_streams * sizeof(StreamPush)));
            if (!st->h_desc[k]) throw std::runtime_error("page-locked descriptors of a stream set");
            st->d_desc[k].alloc((size_t)n_streams);
            HIP_TRY(hipEventCreateWithFlags(&st->desc_free[k], hipEventDisableTiming));
            if (g.held || g.vad) {
                st->h_rdesc[k] = static_cast<RowPush *>(ctu_host_alloc((size_t)n_streams * sizeof(RowPush)));
                if (!st->h_rdesc[k]) throw std::runtime_error("page-locked descriptors of a stream set");
                st->d_rdesc[k].alloc((size_t)n_streams);
            }
        }
        if (g.chained) {
            // by the kernel that runs: [2][64 NJ] of xstate_t (frontend_kernel.h), [2][64 * 9] floats (wave1k_kernel.h), [2][256 NB] floats (bigfft_kernel.h)
            // (subtraction state: the slot of layout_constants.h - both noise estimates and the detector's record)
            const size_t per_stream = ss_set ? (size_t)xs_ss_floats(e->tab.sel.mode == 1 ? 3 : 5)
                                      : !e->tab.big ? (size_t)2 * 64 * (e->tab.sel.mode == 1 ? 3 : 5) * (CTU_EXTEN_F64 ? 2 : 1)
                                      : e->tab.path == BIG_WAVE1K ? (size_t)2 * 64 * 9 : (size_t)2 * 256 * (big_nit(e) / 2 + 1);
            st->xstate.alloc((size_t)n_streams * per_stream);
            HIP_TRY(hipMemset(st->xstate.p, 0, st->xstate.n * sizeof(float)));  // (never read ahead of a store: a file's first tile resets)
            pl->tile_utt.alloc(pl->tiles.n);
            HIP_TRY(hipMemset(pl->tile_utt.p, 0, pl->tile_utt.n * sizeof(int)));
            for (int k = 0; k < 2; k++) {
                st->h_heads[k] = static_cast<int *>(ctu_host_alloc(n_heads * sizeof(int)));
                if (!st->h_heads[k]) throw std::runtime_error("page-locked descriptors of a stream set");
                st->d_heads[k].alloc(n_heads);
            }
        }
        if (st->vad) {
            const int64_t ro = pl->hp.total_frames;
            st->vstate.alloc((size_t)n_streams * VST_DOUBLES);
            HIP_TRY(hipMemset(st->vstate.p, 0, st->vstate.n * sizeof(double)));  // (never read ahead of a store: a file's first push resets)
            st->vsink.alloc((size_t)std::max<int64_t>(ro + (int64_t)n_streams * g.H, 1));
            if (g.held) st->vbase.alloc((size_t)std::max<int64_t>(ro, 1) * d.D);
            for (int k = 0; k < 2; k++) {
                st->h_replay[k] = static_cast<int *>(ctu_host_alloc((size_t)n_streams * sizeof(int)));
                if (!st->h_replay[k]) throw std::runtime_error("page-locked descriptors of a stream set");
                st->d_replay[k].alloc((size_t)n_streams);
            }
        }
        if (st->signal) {
            st->otail.alloc((size_t)n_streams * st->tstride);
            HIP_TRY(hipMemset(st->otail.p, 0, st->otail.n * sizeof(double)));  // (+0.0: a file's first frames add to nothing)
            for (int k = 0; k < 2; k++) {
                st->h_sdesc[k] = static_cast<SignalPush *>(ctu_host_alloc((size_t)n_streams * sizeof(SignalPush)));
                if (!st->h_sdesc[k]) throw std::runtime_error("page-locked descriptors of a stream set");
                st->d_sdesc[k].alloc((size_t)n_streams);
            }
        }
        if (g.held) {
            st->hist.alloc(std::max<size_t>((size_t)2 * n_streams * st->C * st->hw, 1));
            st->means.alloc((size_t)n_streams * STREAM_MEANS);
            HIP_TRY(hipMemset(st->hist.p, 0, st->hist.n * sizeof(float)));
            HIP_TRY(hipMemset(st->means.p, 0, st->means.n * sizeof(float)));
        }
        if (st->trap) {  // a column per row that goes out: no more than the frames of a push, or the half a finish delivers
            const size_t n_cols = (size_t)std::max<int64_t>(pl->hp.total_frames, g.H);
            for (int k = 0; k < 2; k++) {
                st->h_cols[k] = static_cast<int *>(ctu_host_alloc(n_cols * sizeof(int)));
                if (!st->h_cols[k]) throw std::runtime_error("page-locked descriptors of a stream set");
                st->d_cols[k].alloc(n_cols);
            }
        }
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
    if (!st || id < 0 || id >= st->n_streams) return CTU_ERR_INPUT;
    const ctu::Design &d = *st->eng->design;
    return stream_rows_of(st, stream_frames(st->consumed[(size_t)id], d.window, d.wshift));
}

int64_t ctu_streams_pending(const ctu_streams *st, int32_t id) {
    if (!st || id < 0 || id >= st->n_streams) return CTU_ERR_INPUT;
    const ctu::Design &d = *st->eng->design;
    const int64_t F = stream_frames(st->consumed[(size_t)id], d.window, d.wshift);
    if (st->signal) return signal_pending(d, F);
    return F - stream_rows_of(st, F);
}

int64_t ctu_streams_signal_step(int32_t window, int32_t wshift, int64_t total, int64_t *pending) {
    if (window < 1 || wshift < 1 || wshift > window || total < 0) return CTU_ERR_INPUT;
    const int64_t F = stream_frames(total, window, wshift);
    if (pending) *pending = F > 0 ? window - wshift : 0;
    return F * wshift;
}

namespace {
// The row kernels of a push, or of a finish, over the n streams h_rdesc[k] describes (uploaded here); `most` is the largest row count among them
void launch_stream_rows(ctu_streams *st, int k, int n, int64_t most, bool finishing, float *d_rows, hipStream_t s) {
    const ctu::Design &d = *st->eng->design;
    HIP_TRY(hipMemcpyAsync(st->d_rdesc[k].p, st->h_rdesc[k], (size_t)n * sizeof(RowPush), hipMemcpyHostToDevice, s));
    if (most == 0) return;
    RowParams rp;
    rp.push = st->d_rdesc[k].p; rp.fresh = st->plan->base_rows.p; rp.hist = st->hist.p; rp.means = st->means.p; rp.rows = d_rows;
    rp.n_streams = st->n_streams; rp.C = st->C; rp.Dbase = d.Dbase; rp.finishing = finishing ? 1 : 0;
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
// stream_trap_kernel over the rows that go out with a push, or with a finish, of the n streams h_rdesc[k] describes (uploaded here, with
// the stream of every column)
void launch_stream_trap(ctu_streams *st, int k, int n, float *d_rows, hipStream_t s) {
    const ctu::Design &d = *st->eng->design;
    HIP_TRY(hipMemcpyAsync(st->d_rdesc[k].p, st->h_rdesc[k], (size_t)n * sizeof(RowPush), hipMemcpyHostToDevice, s));
    const int64_t n_cols = stream_trap_columns(st->h_rdesc[k], n, st->h_cols[k]);
    if (n_cols == 0) return;
    HIP_TRY(hipMemcpyAsync(st->d_cols[k].p, st->h_cols[k], (size_t)n_cols * sizeof(int), hipMemcpyHostToDevice, s));
    StreamTrapParams tp;
    tp.push = st->d_rdesc[k].p; tp.col = st->d_cols[k].p; tp.fresh = st->plan->logmel.p; tp.hist = st->hist.p; tp.G = st->eng->trapG.p; tp.rows = d_rows;
    tp.n_cols = n_cols; tp.n_streams = st->n_streams; tp.C = st->C; tp.B = d.B;
    tp.traplen = d.o.fea_trapdct_traplen; tp.ndct = d.o.fea_trapdct_ndct; tp.D = d.D;
    const int nrb = tp.ndct <= 16 ? 1 : 2, bb = nrb == 1 ? 8 : 4;
    const dim3 grid((unsigned)((n_cols + 15) / 16), (unsigned)((d.B + bb - 1) / bb));
    const bool comp = (tp.traplen + 3) / 4 > TRAP_COMP_STEPS;  // (contexts of more than 104 frames: stream_trap_kernels.h)
    lift<1, 2>(nrb, [&](auto v) {
        lift<0, 1>(comp, [&](auto c) { hipLaunchKernelGGL((stream_trap_kernel<decltype(v)::value, decltype(c)::value != 0>), grid, dim3(64), 0, s, tp); });
    });
    HIP_TRY(hipGetLastError());
}
// The detector's kernels of a push over the n streams h_rdesc[k] describes and the L.n_replay of them h_replay[k] lists (both uploaded
// here): the replay from every stream's record, then the rows the majority filter releases with the decisions
void launch_stream_vad(ctu_streams *st, int k, int n, const PushLayout &L, float *d_rows, uint8_t *d_vad, hipStream_t s) {
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const ctu_plan *pl = st->plan.get();
    HIP_TRY(hipMemcpyAsync(st->d_rdesc[k].p, st->h_rdesc[k], (size_t)n * sizeof(RowPush), hipMemcpyHostToDevice, s));
    if (L.n_replay == 0) return;
    HIP_TRY(hipMemcpyAsync(st->d_replay[k].p, st->h_replay[k], (size_t)L.n_replay * sizeof(int), hipMemcpyHostToDevice, s));
    StreamVadParams vp;
    vp.push = st->d_rdesc[k].p; vp.replay = st->d_replay[k].p; vp.n_replay = L.n_replay;
    vp.cf = pl->vad_cf.p; vp.ci = pl->vad_ci.p; vp.energy = pl->pnr.p;
    vp.vstate = st->vstate.p; vp.vad = d_vad ? d_vad : st->vsink.p;
    if (e->geom.vad_fused)
        lift<0, 1, 2, 3>(e->vp.thr, [&](auto thr) {
            hipLaunchKernelGGL((stream_vad_lanes_kernel<VF_NC, decltype(thr)::value>), dim3((unsigned)((L.n_replay + 15) / 16)), dim3(64), 0, s, vp, e->vp);
        });
    else hipLaunchKernelGGL(stream_vad_decide_kernel, dim3((unsigned)n), dim3(64), 0, s, vp, e->vp);
    if (st->g.held && L.most > 0) {
        RowParams rp;
        std::memset(&rp, 0, sizeof rp);
        rp.push = st->d_rdesc[k].p; rp.fresh = st->vbase.p; rp.hist = st->hist.p; rp.rows = d_rows;
        rp.n_streams = st->n_streams; rp.C = st->C; rp.Dbase = d.Dbase;
        hipLaunchKernelGGL(stream_vad_rows_kernel, dim3((unsigned)((L.most + 63) / 64), (unsigned)n), dim3(256), 0, s, rp, d.D);
    }
    HIP_TRY(hipGetLastError());
}
// The wrong call for the set, refused before anything changes
constexpr const char *SIGNAL_SET_ROW_CALL = "a set with signal state (CTU_STREAMS_SIGNAL_STATE) delivers samples, not rows: use ctu_streams_push_signal / ctu_streams_finish_signal";
constexpr const char *ROW_SET_SIGNAL_CALL = "ctu_streams_push_signal / ctu_streams_finish_signal need a set with signal state (CTU_STREAMS_SIGNAL_STATE on a configuration with -format_out raw | wave): use ctu_streams_push / ctu_streams_finish";
// The argument checks the device and the host form of a push share (each refuses in its own words)
bool push_args_ok(const ctu_streams *st, int32_t n, const int32_t *ids, const int64_t *n_samples) { return n >= 0 && n <= st->n_streams && (!n || (ids && n_samples)); }
bool push_count_ok(const ctu_streams *st, int64_t n_samples) { return n_samples >= 0 && n_samples <= st->max_push; }
}  // namespace

int ctu_streams_push(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                     float *d_rows, int64_t rows_capacity, int64_t *row_counts, void *stream) {
    return ctu_streams_push_vad(st, n, ids, d_pcm, sample_off, n_samples, d_rows, rows_capacity, row_counts, nullptr, stream);
}

int ctu_streams_push_vad(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                         float *d_rows, int64_t rows_capacity, int64_t *row_counts, uint8_t *d_vad, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const ctu_plan *pl = st->plan.get();
    auto refuse = [&](const char *m) {
        set_error(e, std::string("ENGINE: ") + m);
        return CTU_ERR_INPUT;
    };
    // ---- everything that can be refused is refused here, ahead of the first launch and of any change to the set
    if (st->signal) return refuse(SIGNAL_SET_ROW_CALL);
    if (d_vad && !st->vad) return refuse("push: decisions asked of a set without detector state (CTU_STREAMS_VAD_STATE on a configuration with the VAD module)");
    if (!push_args_ok(st, n, ids, n_samples)) return refuse("push: bad stream count or null argument");
    if (n == 0) return CTU_OK;
    if (++st->push_no == 0) {  // (the counter wrapped: forget the marks)
        std::fill(st->seen.begin(), st->seen.end(), 0u);
        st->push_no = 1;
    }
    int64_t rows = 0, fresh = 0;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= st->n_streams) return refuse("push: stream id out of range");
        if (st->seen[(size_t)ids[i]] == st->push_no) return refuse("push: a stream id appears twice");
        st->seen[(size_t)ids[i]] = st->push_no;
        if (!push_count_ok(st, n_samples[i])) return refuse("push: more samples than the set's max_push_samples (or fewer than none)");
        if (n_samples[i] && (!sample_off || sample_off[i] < 0)) return refuse("push: null or negative sample offsets");
        const int64_t c = st->consumed[(size_t)ids[i]];
        rows += stream_rows_of(st, stream_frames(c + n_samples[i], d.window, d.wshift)) - stream_rows_of(st, stream_frames(c, d.window, d.wshift));
        fresh += n_samples[i];
    }
    if (fresh && !d_pcm) return refuse("push: null sample buffer");
    if (rows > rows_capacity || (rows && !d_rows)) return refuse("push: the rows of this push do not fit rows_capacity");
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const int k = st->turn;
        HIP_TRY(hipEventSynchronize(st->desc_free[k]));  // (the push before last has read them; immediate before the first record)
        // ---- plan: the whole push, into this turn's page-locked descriptors and the set's scratch; the set itself is only read
        PushLayout L;
        L.push = st->h_desc[k]; L.rows = st->h_rdesc[k]; L.heads = st->h_heads[k]; L.tail = st->chain_tail.data();
        L.row_counts = row_counts ? row_counts : st->counts.data();  // (the caller's array is output of the call: planned in place)
        L.consumed = st->next_consumed.data(); L.hsel = st->next_hsel.data(); L.replay = st->h_replay[k];
        if (!stream_plan_push(st->g, st->consumed.data(), st->hsel.data(), n, ids, n_samples, sample_off, L))
            throw std::runtime_error("internal: a push beyond the set's arena");
        // ---- commit: nothing refuses this push any more.  The mirrors take their next values; what follows is HIP calls alone
        st->turn ^= 1;
        for (int i = 0; i < n; i++) st->consumed[(size_t)ids[i]] = L.consumed[i];
        if (st->g.held)
            for (int i = 0; i < n; i++) st->hsel[(size_t)ids[i]] = L.hsel[i];
        // ---- launch
        const bool held = st->g.held;
        HIP_TRY(hipMemcpyAsync(st->d_desc[k].p, L.push, (size_t)n * sizeof(StreamPush), hipMemcpyHostToDevice, s));
        RunExtent x;  // the front end and its tails run over the front of the set's plan: this push
        x.n_tiles = L.tiles; x.grid = L.grid; x.total_frames = L.base_rows;
        x.heads = L.n_heads ? st->d_heads[k].p : pl->ext.heads;
        x.n_heads = L.n_heads ? L.n_heads : pl->ext.n_heads;
        x.xstate = st->xstate.p;
        StreamParams sp;
        sp.push = st->d_desc[k].p; sp.state = st->state.p; sp.carry = st->carry.p; sp.arena = st->arena.p; sp.src = d_pcm; sp.tiles = pl->tiles.p;
        sp.cstride = st->cstride; sp.window = d.window; sp.wshift = d.wshift;
        sp.n_tiles = L.tiles; sp.grid = L.grid;
        sp.tile_stream = L.n_heads ? pl->tile_utt.p : nullptr;
        if (L.n_heads) HIP_TRY(hipMemcpyAsync(st->d_heads[k].p, L.heads, (size_t)L.n_heads * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(st->ev[0], s));
        hipLaunchKernelGGL(stream_stitch_kernel, dim3((unsigned)n, (unsigned)L.slices), dim3(256), 0, s, sp);
        HIP_TRY(hipEventRecord(st->ev[1], s));
        HIP_TRY(hipGetLastError());
        int rc = CTU_OK;
        // (held) where the front end leaves the push's rows - with trap state its log-mel rows, and no kernel of the run writes rows
        float *const base = st->trap ? pl->logmel.p : st->vad ? st->vbase.p : pl->base_rows.p;
        if (L.tiles) rc = run_chain(e, pl, x, st->arena.p, held ? base : d_rows, nullptr, s, !held, !st->vad);
        if (st->vad && L.tiles && rc == CTU_OK) launch_stream_vad(st, k, n, L, d_rows, d_vad, s);
        else if (st->trap && L.tiles && rc == CTU_OK) launch_stream_trap(st, k, n, d_rows, s);
        else if (held && L.tiles && rc == CTU_OK) launch_stream_rows(st, k, n, L.most, false, d_rows, s);
        HIP_TRY(hipEventRecord(st->ev[2], s));
        hipLaunchKernelGGL(stream_carry_kernel, dim3((unsigned)n), dim3(256), 0, s, sp);
        if (held && st->C > 0 && L.tiles && rc == CTU_OK) {
            RowParams rp;
            std::memset(&rp, 0, sizeof rp);
            rp.push = st->d_rdesc[k].p; rp.fresh = base; rp.hist = st->hist.p;
            rp.n_streams = st->n_streams; rp.C = st->C; rp.Dbase = st->hw;
            hipLaunchKernelGGL(stream_rows_carry_kernel, dim3((unsigned)n, (unsigned)((st->C * st->hw + 255) / 256)), dim3(256), 0, s, rp);
        }
        HIP_TRY(hipEventRecord(st->ev[3], s));
        HIP_TRY(hipEventRecord(st->desc_free[k], s));
        HIP_TRY(hipGetLastError());
        st->timed = true;
        return rc;
    });
}

int ctu_streams_push_host(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples, float *h_rows,
                          int64_t rows_capacity, int64_t *row_counts) {
    return ctu_streams_push_vad_host(st, n, ids, h_pcm, n_samples, h_rows, rows_capacity, row_counts, nullptr);
}

int ctu_streams_push_vad_host(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples, float *h_rows,
                              int64_t rows_capacity, int64_t *row_counts, uint8_t *h_vad) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    if (st->signal) {
        set_error(e, std::string("ENGINE: ") + SIGNAL_SET_ROW_CALL);
        return CTU_ERR_INPUT;
    }
    if (h_vad && !st->vad) {
        set_error(e, "ENGINE: push: decisions asked of a set without detector state (CTU_STREAMS_VAD_STATE on a configuration with the VAD module)");
        return CTU_ERR_INPUT;
    }
    const int D = e->design->D;
    if (!push_args_ok(st, n, ids, n_samples) || (n && !h_pcm)) {
        set_error(e, "ENGINE: push: bad stream count or null argument");
        return CTU_ERR_INPUT;
    }
    int64_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (!push_count_ok(st, n_samples[i]) || (n_samples[i] && !h_pcm[i])) {
            set_error(e, "ENGINE: push: more samples than the set's max_push_samples (or fewer than none), or a null sample buffer");
            return CTU_ERR_INPUT;
        }
        fresh += n_samples[i];
    }
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const size_t cap = (size_t)st->n_streams * (size_t)st->max_push;
        if (!st->h_stage) {
            st->h_stage = static_cast<int16_t *>(ctu_host_alloc(cap * sizeof(int16_t)));
            if (!st->h_stage) throw std::runtime_error("page-locked staging of a stream set");
            st->d_stage.alloc(cap);
            // (a push that brings a stream's frame wmax + 2 also delivers the rows of the wmax + 1 frames before it)
            st->d_rows.alloc((size_t)std::max<int64_t>(st->plan->hp.total_frames + (int64_t)st->n_streams * (st->g.wmax + 1), 1) * D);
        }
        int64_t at = 0;
        for (int i = 0; i < n; i++) {
            st->offs[(size_t)i] = at;
            if (n_samples[i]) std::memcpy(st->h_stage + at, h_pcm[i], (size_t)n_samples[i] * sizeof(int16_t));
            at += n_samples[i];
        }
        if (fresh) HIP_TRY(hipMemcpyAsync(st->d_stage.p, st->h_stage, (size_t)fresh * sizeof(int16_t), hipMemcpyHostToDevice, nullptr));
        // the device rows hold any push of the set; what the caller's buffer holds is the device form's check
        const int rc = ctu_streams_push_vad(st, n, ids, st->d_stage.p, st->offs.data(), n_samples, h_rows ? st->d_rows.p : nullptr, h_rows ? rows_capacity : 0,
                                            row_counts, h_vad ? st->vsink.p : nullptr, nullptr);
        if (rc != CTU_OK) return rc;
        const int64_t *counts = row_counts ? row_counts : st->counts.data();  // (where the push planned them)
        int64_t rows = 0;
        for (int i = 0; i < n; i++) rows += counts[i];
        if (rows) {  // page-locked rows at the link rate, pageable ones through the runtime's staging (as run_host_ranges downloads)
            if (is_pinned(h_rows)) HIP_TRY(hipMemcpyAsync(h_rows, st->d_rows.p, (size_t)rows * D * 4, hipMemcpyDeviceToHost, nullptr));
            else HIP_TRY(hipMemcpy(h_rows, st->d_rows.p, (size_t)rows * D * 4, hipMemcpyDeviceToHost));
            if (h_vad) HIP_TRY(hipMemcpyAsync(h_vad, st->vsink.p, (size_t)rows, hipMemcpyDeviceToHost, nullptr));
        }
        HIP_TRY(hipStreamSynchronize(nullptr));
        return CTU_OK;
    });
}

int ctu_streams_finish(ctu_streams *st, int32_t id, float *d_rows, int64_t rows_capacity, int64_t *row_count, void *stream) {
    return ctu_streams_finish_vad(st, id, d_rows, rows_capacity, row_count, nullptr, stream);
}

int ctu_streams_finish_vad(ctu_streams *st, int32_t id, float *d_rows, int64_t rows_capacity, int64_t *row_count, uint8_t *d_vad, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    if (st->signal) {
        set_error(e, std::string("ENGINE: ") + SIGNAL_SET_ROW_CALL);
        return CTU_ERR_INPUT;
    }
    if (d_vad && !st->vad) {
        set_error(e, "ENGINE: finish: decisions asked of a set without detector state (CTU_STREAMS_VAD_STATE on a configuration with the VAD module)");
        return CTU_ERR_INPUT;
    }
    if (id < 0 || id >= st->n_streams) {
        set_error(e, "ENGINE: finish: stream id out of range");
        return CTU_ERR_INPUT;
    }
    if (row_count) *row_count = 0;  // fread() comes up short on a trailing partial window and the file ends there (src/io/in.cc:314,438)
    const int64_t total = st->consumed[(size_t)id];
    const FinishLayout fin = stream_plan_finish(d.window, d.wshift, st->g.H, st->g.wmax, total, id, st->hsel[(size_t)id], st->vad);
    const int64_t pending = fin.pending;
    const bool too_short = fin.too_short;
    if (pending > rows_capacity || (pending && !d_rows)) {  // ahead of any launch or change: the stream stays as it was
        set_error(e, "ENGINE: finish: the rows held back for this stream do not fit rows_capacity");
        return CTU_ERR_INPUT;
    }
    st->consumed[(size_t)id] = 0;
    hipStream_t s = (hipStream_t)stream;
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        if (pending) {  // rows r0 .. F - 1 with the file's length known: every base row they read is in the history
            const int k = st->turn;
            st->turn ^= 1;
            HIP_TRY(hipEventSynchronize(st->desc_free[k]));
            st->h_rdesc[k][0] = fin.row;
            if (st->vad) {  // the filter's flush and the h rows it releases, with the file's length known
                HIP_TRY(hipMemcpyAsync(st->d_rdesc[k].p, st->h_rdesc[k], sizeof(RowPush), hipMemcpyHostToDevice, s));
                RowParams rp;
                std::memset(&rp, 0, sizeof rp);
                rp.push = st->d_rdesc[k].p; rp.hist = st->hist.p; rp.rows = d_rows;
                rp.n_streams = st->n_streams; rp.C = st->C; rp.Dbase = d.Dbase; rp.finishing = 1;
                hipLaunchKernelGGL(stream_vad_finish_kernel, dim3(1), dim3(256), 0, s, rp, d.D, st->vstate.p, d_vad, d.o.vad_filter_order);
                HIP_TRY(hipGetLastError());
            } else if (st->trap) launch_stream_trap(st, k, 1, d_rows, s);  // (Tn = 0: the newest frame is the file's last)
            else launch_stream_rows(st, k, 1, pending, true, d_rows, s);
            HIP_TRY(hipEventRecord(st->desc_free[k], s));
        }
        HIP_TRY(hipMemsetAsync(st->state.p + id, 0, sizeof(StreamState), s));
        if (st->g.held && !st->vad) HIP_TRY(hipMemsetAsync(st->means.p + (size_t)id * STREAM_MEANS, 0, STREAM_MEANS * sizeof(float), s));
        if (st->trap)  // both histories of the stream (a new file reads neither ahead of its own rows: the left clamp is frame 0)
            for (int h = 0; h < 2; h++)
                HIP_TRY(hipMemsetAsync(st->hist.p + ((size_t)h * st->n_streams + id) * st->C * st->hw, 0, (size_t)st->C * st->hw * sizeof(float), s));
        return CTU_OK;
    });
    if (rc != CTU_OK) return rc;
    if (total > 0 && total < d.window - d.wshift) {
        set_error(e, "IO: Signal shorter than one frame!");  // src/io/in.cc:277; the stream is reset all the same
        return CTU_ERR_INPUT;
    }
    if (too_short && st->trap) {  // the words of an offline plan's refusal (plan.cc); the stream is reset all the same
        set_error(e, "ENGINE: trapdct on fewer than (traplen+1)/2 frames is undefined in the reference (src/fea/fea_trap.cc:64-70)");
        return CTU_ERR_INPUT;
    }
    if (too_short) {  // the same for a delta chain or a stacking
        set_error(e, "ENGINE: delta / stacking on fewer than window+2 frames is ill-defined in the reference (src/fea/fea_delta.cc:74-130,178-206)");
        return CTU_ERR_INPUT;
    }
    if (row_count) *row_count = pending;
    return CTU_OK;
}

int ctu_streams_finish_host(ctu_streams *st, int32_t id, float *h_rows, int64_t rows_capacity, int64_t *row_count) {
    return ctu_streams_finish_vad_host(st, id, h_rows, rows_capacity, row_count, nullptr);
}

int ctu_streams_finish_vad_host(ctu_streams *st, int32_t id, float *h_rows, int64_t rows_capacity, int64_t *row_count, uint8_t *h_vad) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    if (st->signal) {
        set_error(e, std::string("ENGINE: ") + SIGNAL_SET_ROW_CALL);
        return CTU_ERR_INPUT;
    }
    if (h_vad && !st->vad) {
        set_error(e, "ENGINE: finish: decisions asked of a set without detector state (CTU_STREAMS_VAD_STATE on a configuration with the VAD module)");
        return CTU_ERR_INPUT;
    }
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

// ---- signal state: the same push - check, plan, commit, launch - with samples out.  The front end leaves the time-domain frames of the
// push in the plan's ybuf, a row per frame (its SY instantiations; in a build without them synth_kernel from the exported spectra), and
// stream_ola_kernel adds them onto every stream's tail.  With CTU_STREAMS_LARGE_STATE on 1024 .. 4096-point frames the frames come from
// bigfft_kernel's exported spectra through bigsynth_kernel, and a tail of more than OLA_TAIL_MAX entries is stream_ola_big_kernel's.
namespace {
SignalParams signal_params(const ctu_streams *st, const SignalPush *push, int16_t *d_out) {
    const ctu::Design &d = *st->eng->design;
    SignalParams gp;
    gp.push = push; gp.ybuf = st->plan->ybuf.p; gp.tail = st->otail.p; gp.out = d_out;
    gp.tstride = st->tstride; gp.window = d.window; gp.wshift = d.wshift;
    gp.corr = d.ola_corr;
    return gp;
}
}  // namespace

int ctu_streams_push_signal(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *d_pcm, const int64_t *sample_off, const int64_t *n_samples,
                            int16_t *d_out, int64_t out_capacity, int64_t *out_counts, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    const ctu_plan *pl = st->plan.get();
    auto refuse = [&](const char *m) {
        set_error(e, std::string("ENGINE: ") + m);
        return CTU_ERR_INPUT;
    };
    // ---- everything that can be refused is refused here or by the plan, ahead of the first launch and of any change to the set
    if (!st->signal) return refuse(ROW_SET_SIGNAL_CALL);
    if (!push_args_ok(st, n, ids, n_samples)) return refuse("push: bad stream count or null argument");
    if (n == 0) return CTU_OK;
    if (++st->push_no == 0) {  // (the counter wrapped: forget the marks)
        std::fill(st->seen.begin(), st->seen.end(), 0u);
        st->push_no = 1;
    }
    int64_t fresh = 0, out = 0;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= st->n_streams) return refuse("push: stream id out of range");
        if (st->seen[(size_t)ids[i]] == st->push_no) return refuse("push: a stream id appears twice");
        st->seen[(size_t)ids[i]] = st->push_no;
        if (!push_count_ok(st, n_samples[i])) return refuse("push: more samples than the set's max_push_samples (or fewer than none)");
        if (n_samples[i] && (!sample_off || sample_off[i] < 0)) return refuse("push: null or negative sample offsets");
        const int64_t c = st->consumed[(size_t)ids[i]];
        out += (stream_frames(c + n_samples[i], d.window, d.wshift) - stream_frames(c, d.window, d.wshift)) * d.wshift;
        fresh += n_samples[i];
    }
    if (fresh && !d_pcm) return refuse("push: null sample buffer");
    if (out_capacity < 0 || (out && !d_out)) return refuse("push: the samples of this push do not fit out_capacity");
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const int k = st->turn;
        HIP_TRY(hipEventSynchronize(st->desc_free[k]));  // (the push before last has read them; immediate before the first record)
        // ---- plan: as ctu_streams_push plans, with the samples' prefix sums and the capacity check (stream_plan.h)
        PushLayout L;
        L.push = st->h_desc[k]; L.sig = st->h_sdesc[k]; L.heads = st->h_heads[k]; L.tail = st->chain_tail.data();
        L.row_counts = out_counts ? out_counts : st->counts.data();
        L.consumed = st->next_consumed.data(); L.hsel = st->next_hsel.data();
        L.capacity = out_capacity;
        if (!stream_plan_push(st->g, st->consumed.data(), st->hsel.data(), n, ids, n_samples, sample_off, L)) {
            if (L.over_capacity) return refuse("push: the samples of this push do not fit out_capacity");
            throw std::runtime_error("internal: a push beyond the set's arena");
        }
        // ---- commit
        st->turn ^= 1;
        for (int i = 0; i < n; i++) st->consumed[(size_t)ids[i]] = L.consumed[i];
        // ---- launch
        HIP_TRY(hipMemcpyAsync(st->d_desc[k].p, L.push, (size_t)n * sizeof(StreamPush), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st->d_sdesc[k].p, L.sig, (size_t)n * sizeof(SignalPush), hipMemcpyHostToDevice, s));
        RunExtent x;
        x.n_tiles = L.tiles; x.grid = L.grid; x.total_frames = L.base_rows;
        x.heads = L.n_heads ? st->d_heads[k].p : pl->ext.heads;
        x.n_heads = L.n_heads ? L.n_heads : pl->ext.n_heads;
        x.xstate = st->xstate.p;
        StreamParams sp;
        sp.push = st->d_desc[k].p; sp.state = st->state.p; sp.carry = st->carry.p; sp.arena = st->arena.p; sp.src = d_pcm; sp.tiles = pl->tiles.p;
        sp.cstride = st->cstride; sp.window = d.window; sp.wshift = d.wshift;
        sp.n_tiles = L.tiles; sp.grid = L.grid;
        sp.tile_stream = L.n_heads ? pl->tile_utt.p : nullptr;
        if (L.n_heads) HIP_TRY(hipMemcpyAsync(st->d_heads[k].p, L.heads, (size_t)L.n_heads * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(st->ev[0], s));
        hipLaunchKernelGGL(stream_stitch_kernel, dim3((unsigned)n, (unsigned)L.slices), dim3(256), 0, s, sp);
        HIP_TRY(hipEventRecord(st->ev[1], s));
        HIP_TRY(hipGetLastError());
        int rc = CTU_OK;
        if (L.tiles) {
            e->in_signal_call = true;
            rc = run_chain(e, pl, x, st->arena.p, nullptr, nullptr, s, true);
            e->in_signal_call = false;
        }
        if (L.tiles && rc == CTU_OK) {
            if (e->tab.big) launch_bigsynth(e, pl, x, s, 1.0f / (float)d.wfft);  // (large transforms: bigfft_kernel exported the spectra)
            else if (!e->tab.sel.sy) {  // the spectra of the push's frames back to the time domain (ctu_engine_run_signal's launch, over this extent)
                SynthParams yp;
                yp.K = d.K; yp.wfft = d.wfft; yp.window = d.window; yp.wshift = d.wshift;
                yp.inv_n = 1.0f / (float)d.wfft;
                yp.corr = d.ola_corr;
                const int g = (int)std::min<int64_t>((L.base_rows + 7) / 8, (int64_t)e->n_cu * 8);
                hipLaunchKernelGGL(synth_kernel, dim3(g), dim3(256), 0, s, pl->xri.p, pl->pnr.p, pl->ybuf.p, (long long)L.base_rows, yp);
            }
            if (st->ola_big) {  // the owner of every tail, then the slices of the samples past it
                const int64_t past = std::max<int64_t>(L.most - (d.window - d.wshift), 0);
                hipLaunchKernelGGL(stream_ola_big_kernel, dim3((unsigned)n, 1u + (unsigned)((past + OLA_SLICE - 1) / OLA_SLICE)), dim3(256), 0, s,
                                   signal_params(st, st->d_sdesc[k].p, d_out));
            } else {
                const unsigned slices = (unsigned)((L.most + OLA_SLICE - 1) / OLA_SLICE);
                hipLaunchKernelGGL(stream_ola_kernel, dim3((unsigned)n, slices), dim3(256), 0, s, signal_params(st, st->d_sdesc[k].p, d_out));
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(st->ev[2], s));
        hipLaunchKernelGGL(stream_carry_kernel, dim3((unsigned)n), dim3(256), 0, s, sp);
        HIP_TRY(hipEventRecord(st->ev[3], s));
        HIP_TRY(hipEventRecord(st->desc_free[k], s));
        HIP_TRY(hipGetLastError());
        st->timed = true;
        return rc;
    });
}

int ctu_streams_push_signal_host(ctu_streams *st, int32_t n, const int32_t *ids, const int16_t *const *h_pcm, const int64_t *n_samples, int16_t *h_out,
                                 int64_t out_capacity, int64_t *out_counts) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    if (!st->signal) {
        set_error(e, std::string("ENGINE: ") + ROW_SET_SIGNAL_CALL);
        return CTU_ERR_INPUT;
    }
    if (!push_args_ok(st, n, ids, n_samples) || (n && !h_pcm)) {
        set_error(e, "ENGINE: push: bad stream count or null argument");
        return CTU_ERR_INPUT;
    }
    int64_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (!push_count_ok(st, n_samples[i]) || (n_samples[i] && !h_pcm[i])) {
            set_error(e, "ENGINE: push: more samples than the set's max_push_samples (or fewer than none), or a null sample buffer");
            return CTU_ERR_INPUT;
        }
        fresh += n_samples[i];
    }
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const size_t cap = (size_t)st->n_streams * (size_t)st->max_push;
        if (!st->h_stage) {
            st->h_stage = static_cast<int16_t *>(ctu_host_alloc(cap * sizeof(int16_t)));
            if (!st->h_stage) throw std::runtime_error("page-locked staging of a stream set");
            st->d_stage.alloc(cap);
            // (a stream delivers wshift samples per frame, and a push completes frames out of its own samples and fewer than `window` carried ones)
            st->d_sig.alloc((size_t)st->n_streams * ((size_t)st->max_push + (size_t)e->design->window));
        }
        int64_t at = 0;
        for (int i = 0; i < n; i++) {
            st->offs[(size_t)i] = at;
            if (n_samples[i]) std::memcpy(st->h_stage + at, h_pcm[i], (size_t)n_samples[i] * sizeof(int16_t));
            at += n_samples[i];
        }
        if (fresh) HIP_TRY(hipMemcpyAsync(st->d_stage.p, st->h_stage, (size_t)fresh * sizeof(int16_t), hipMemcpyHostToDevice, nullptr));
        // the device samples hold any push of the set; what the caller's buffer holds is the device form's check
        const int rc = ctu_streams_push_signal(st, n, ids, st->d_stage.p, st->offs.data(), n_samples, h_out ? st->d_sig.p : nullptr, h_out ? out_capacity : 0,
                                               out_counts, nullptr);
        if (rc != CTU_OK) return rc;
        const int64_t *counts = out_counts ? out_counts : st->counts.data();  // (where the push planned them)
        int64_t out = 0;
        for (int i = 0; i < n; i++) out += counts[i];
        if (out) HIP_TRY(hipMemcpyAsync(h_out, st->d_sig.p, (size_t)out * sizeof(int16_t), hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return CTU_OK;
    });
}

int ctu_streams_finish_signal(ctu_streams *st, int32_t id, int16_t *d_out, int64_t out_capacity, int64_t *out_count, void *stream) {
    if (!st) return CTU_ERR_INPUT;
    ctu_engine *e = st->eng;
    const ctu::Design &d = *e->design;
    if (!st->signal) {
        set_error(e, std::string("ENGINE: ") + ROW_SET_SIGNAL_CALL);
        return CTU_ERR_INPUT;
    }
    if (id < 0 || id >= st->n_streams) {
        set_error(e, "ENGINE: finish: stream id out of range");
        return CTU_ERR_INPUT;
    }
    if (out_count) *out_count = 0;
    const int64_t total = st->consumed[(size_t)id];
    const FinishLayout fin = stream_plan_finish(d.window, d.wshift, 0, 0, total, id, 0, false, true);
    if (fin.pending > out_capacity || (fin.pending && !d_out)) {  // ahead of any launch or change: the stream stays as it was
        set_error(e, "ENGINE: finish: the samples of this stream's tail do not fit out_capacity");
        return CTU_ERR_INPUT;
    }
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
    if (!st->signal) {
        set_error(e, std::string("ENGINE: ") + ROW_SET_SIGNAL_CALL);
        return CTU_ERR_INPUT;
    }
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

