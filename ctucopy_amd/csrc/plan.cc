// The plan of an offline run, worked out on the host before anything reaches the device (plan_host.h): where every utterance sits in
// the arena and in the rows, the refusals, the tiles and the chains the front end walks, the lists the later stages read, how large
// every scratch buffer is.  Host only, HIP-free: index arithmetic over PlanGeom and the constants of layout_constants.h.  Every
// kernel trusts these numbers blindly; engine.hip uploads and allocates by them and decides nothing itself.
#include "plan_host.h"

#include <algorithm>
#include <queue>
#include <utility>

#include "stream_plan.h"  // chain_deal: where chain c sits among the chain heads (a push deals streams by the same rule)

namespace ctu {

PlanGeom plan_geom(const Design &d, const EngineTables &tab, const Spread &sp, int n_cu) {
    static_assert(TILE == 64, "the chunk list of the TRAP / delta / CMS / CMVN passes (64 frames per workgroup) is the tile list");
    const Opts &o = d.o;
    PlanGeom g;
    g.rows_in = d.rows_in;
    g.window = d.window; g.wshift = d.wshift; g.Dbase = d.Dbase; g.D = d.D; g.K = d.K; g.B = d.B;
    g.post_order = d.post_order;
    for (int j = 0; j < d.post_order; j++) g.post_wmax = std::max(g.post_wmax, d.post_w[j]);
    g.rows_grid_cap = n_cu * ROWS_WG_PER_CU;
    g.chunked = d.rows_in || d.kind == FeaKind::TrapDct || d.post_order > 0 || d.cms || o.stat_cmvn || o.apply_cmvn;
    g.staged = d.post_order > 0 || d.cms;
    if (d.rows_in) return g;  // what follows serves the front end and the stages that read its scratch
    const FeSel &k = tab.sel;
    g.trap_min = d.kind == FeaKind::TrapDct ? (o.fea_trapdct_traplen + 1) / 2 : 0;
    g.per_wave = o.nr_mode == "exten" || tab.ss;
    // two workgroups per CU when the instantiation keeps to 128 VGPRs (four waves per SIMD) and 80 KB of LDS; the synthesis and the
    // 512-point detector instantiations take 256 VGPRs
    g.max_wg = n_cu * ((fe_waves_per_simd(k.mode, k.vf, k.ss, k.sy) >= 4 && tab.lds_bytes <= (size_t)LDS_2WG) ? 2 : 1);
    // (bigfft_kernel and bigss_kernel walk a chain with a whole workgroup of 256 threads: eight of them fit a CU at once)
    g.chain_slots = (tab.big && tab.path != BIG_WAVE1K) ? n_cu * 8 : g.max_wg * NWAVE;
    g.per_utt = d.signal_out || o.remove_dc1;
    const VadParams vp = vad_params(d, sp);
    g.do_vad = o.do_vad();
    g.vad_energy = g.do_vad && vp.cri == 0;
    g.vad_burg = g.do_vad && vp.cri == 1 && !k.vf;
    g.vad_fused = g.do_vad && vp.cri == 1 && k.vf;
    g.vad_ncoef = vp.ncoef;
    g.ss = tab.ss != 0;
    g.ss_big = g.ss && tab.big;
    g.ss_detector = g.ss_big && !tab.ss_file;
    g.ss_ncep = o.fea_ncepcoefs;
    g.row_off_dev = g.do_vad || g.ss_detector;
    g.signal_out = d.signal_out;
    g.pss = g.ss_big && d.signal_out;
    g.spectra = (d.signal_out && !k.sy) || g.vad_burg || g.ss_big;  // (signal output without SY: on 1024- to 4096-point transforms, where fe_select leaves k.sy unset)
    g.dc1 = o.remove_dc1;
    g.logmel = d.kind == FeaKind::TrapDct || tab.dctw;
    g.lp_tail = (tab.feat == FEAT_LP || tab.feat == FEAT_LPD) && (!tab.big || tab.path == BIG_WAVE1K) && !d.signal_out;
    g.lags_double = tab.feat == FEAT_LPD || tab.big;
    g.lporder = o.fea_lporder;
    return g;
}

int64_t arena_layout(const int64_t *utt_nsamples, int32_t n_utt, int64_t *sample_off) {
    if (n_utt < 0 || (n_utt && !utt_nsamples)) return CTU_ERR_INPUT;
    int64_t so = PCM_HEAD;
    for (int i = 0; i < n_utt; i++) {
        if (utt_nsamples[i] < 0) return CTU_ERR_INPUT;
        if (sample_off) sample_off[i] = so;
        so += pcm_slot(utt_nsamples[i]);
    }
    if (sample_off) sample_off[n_utt] = so;
    return so + PCM_TAIL;  // loads run to the end of the last 32-sample row of a frame
}

int64_t rows_arena_layout(const int64_t *utt_rows, int32_t n_utt, int32_t width, int64_t *word_off) {
    if (n_utt < 0 || width < 1 || (n_utt && !utt_rows)) return CTU_ERR_INPUT;
    int64_t wo = 0;
    for (int i = 0; i < n_utt; i++) {
        if (utt_rows[i] < 0) return CTU_ERR_INPUT;
        if (word_off) word_off[i] = wo;
        wo += rows_slot(utt_rows[i] * width);
    }
    if (word_off) word_off[n_utt] = wo;
    return wo;  // rows_ingest_kernel reads an utterance's own words only: no padding around the arena
}

int64_t plan_num_frames(const PlanGeom &g, int64_t n) {
    if (g.rows_in) return n < 0 ? -1 : n;  // the "samples" of a feature file are its rows
    const int pre = g.window - g.wshift;
    if (n < pre) return -1;
    return (n - pre) / g.wshift;
}

namespace {
// Step 1, for both kinds of plan: where every utterance sits in the arena and in the rows, the refusals, its tiles and 64-frame
// chunks, the totals.  The two kinds differ in the arena's layout rule, in what a length counts (plan_num_frames: samples against the
// rows themselves, -format_in htk), in the arena elements between two frames, and in a refusal each.
int plan_layout(const PlanGeom &g, const int64_t *utt_n, int32_t n_utt, HostPlan &h, std::string &err) {
    const bool rows = g.rows_in;
    h.n_utt = n_utt;
    h.nsamples.assign(utt_n, utt_n + n_utt);
    h.sample_off.resize(n_utt + 1);
    h.row_off.resize(n_utt + 1);
    h.frames.resize(n_utt);
    h.total_samples = rows ? rows_arena_layout(utt_n, n_utt, g.Dbase, h.sample_off.data()) : arena_layout(utt_n, n_utt, h.sample_off.data());
    if (h.total_samples < 0) {
        err = "ENGINE: negative utterance length";
        return CTU_ERR_INPUT;
    }
    const int64_t stride = rows ? g.Dbase : g.wshift;  // arena elements from one frame to the next
    const bool info = g.chunked || g.per_utt;
    h.uts.assign(n_utt + 1, 0);
    if (info) h.uinfo.resize(n_utt);
    std::vector<TileRec> tiles;  // local, moved into `h` behind the loop: pushing through `h` measured 3 % on plan creation (profiles/host_pipeline_ab.txt)
    std::vector<int> chunks;
    int64_t ro = 0;
    for (int i = 0; i < n_utt; i++) {
        const int64_t T = plan_num_frames(g, utt_n[i]);
        if (T < 0) {
            err = "IO: Signal shorter than one frame!";  // src/io/in.cc:277
            return CTU_ERR_INPUT;
        }
        if (rows && T > 0x7fffffff / 2) {
            err = "ENGINE: feature file too long";
            return CTU_ERR_INPUT;
        }
        // With exactly window+1 frames a stage never takes its steady-state branch, so its flush starts from ring
        // slot 0 instead of the oldest slot and the emitted rows mix frames (src/fea/fea_delta.cc:118,183-186);
        // with fewer it reads slots that were never written.  Neither is a feature worth reproducing.
        if (g.post_order > 0 && T > 0 && T < g.post_wmax + 2) {
            err = "ENGINE: delta / stacking on fewer than window+2 frames is ill-defined in the reference (src/fea/fea_delta.cc:74-130,178-206)";
            return CTU_ERR_INPUT;
        }
        if (T > 0 && T < g.trap_min) {
            err = "ENGINE: trapdct on fewer than (traplen+1)/2 frames is undefined in the reference (src/fea/fea_trap.cc:64-70)";
            return CTU_ERR_INPUT;
        }
        const int64_t so = h.sample_off[i];
        h.row_off[i] = ro;
        h.frames[i] = T;
        h.uts[i] = (int)tiles.size();
        for (int64_t t0 = 0; t0 < T; t0 += TILE) {
            TileRec r;
            r.sbase = so + t0 * stride;
            r.rbase = ro + t0;
            r.nvalid = (int)std::min<int64_t>(TILE, T - t0);
            r.t0 = (int)t0;
            r.next = -1;
            r.T = (int)T;
            tiles.push_back(r);
            if (g.chunked) {
                chunks.push_back(i);
                chunks.push_back((int)t0);
            }
        }
        if (info) h.uinfo[i] = {(int)(ro & 0xffffffff), (int)(ro >> 32), (int)T, 0};
        h.max_frames = std::max<int>(h.max_frames, (int)T);
        ro += T;
    }
    h.uts[n_utt] = (int)tiles.size();
    h.row_off[n_utt] = ro;
    h.total_frames = ro;
    h.tiles = std::move(tiles);
    h.chunks = std::move(chunks);
    h.n_chunks = (int)h.chunks.size() / 2;
    return CTU_OK;
}

// Step 2, for plans over samples: the chains the front end walks and the grid they are built for.  (A plan over rows has no chains:
// rows_ingest_kernel strides over the tile list, four tiles - one per wave - to a workgroup pass.)
// Each workgroup walks a chain of tiles.  Stateless chains stride over the tile list; with a per-utterance recurrence (exten, the
// *ss modes) a wave takes whole utterances, tile after tile.
void plan_chains(const PlanGeom &g, HostPlan &h) {
    std::vector<TileRec> &tiles = h.tiles;
    const std::vector<int> &uts = h.uts;
    const int n_tiles = (int)tiles.size();
    if (g.per_wave) {
        // whole utterances, longest first onto the least loaded chain (LPT), tile after tile
        std::vector<int> live;  // utterances that have at least one frame
        for (int i = 0; i < h.n_utt; i++)
            if (uts[i + 1] > uts[i]) live.push_back(i);
        std::stable_sort(live.begin(), live.end(), [&](int a, int b) { return h.frames[a] > h.frames[b]; });
        const ChainDeal deal = chain_deal((int)live.size(), g.chain_slots);  // (the chains of one workgroup are spread over the length ranks)
        h.heads.assign((size_t)deal.heads(), -1);
        std::vector<int> tail(deal.C, -1);  // last tile of each chain so far
        std::priority_queue<std::pair<int64_t, int>, std::vector<std::pair<int64_t, int>>, std::greater<std::pair<int64_t, int>>> load;
        for (int c = 0; c < deal.C; c++) load.push({0, c});
        for (int u : live) {
            const auto top = load.top();
            load.pop();
            const int c = top.second;
            for (int t = uts[u]; t + 1 < uts[u + 1]; t++) tiles[t].next = t + 1;
            tiles[uts[u + 1] - 1].next = -1;
            if (tail[c] < 0) h.heads[deal.slot(c)] = uts[u];
            else tiles[tail[c]].next = uts[u];
            tail[c] = uts[u + 1] - 1;
            load.push({top.first + h.frames[u], c});
        }
        h.grid = deal.G;
    } else {
        const int G = std::max(1, std::min(n_tiles, g.max_wg));
        h.heads.assign(G, -1);
        for (int t = 0; t < n_tiles; t++) tiles[t].next = (t + G < n_tiles) ? t + G : -1;
        for (int c = 0; c < G && c < n_tiles; c++) h.heads[c] = c;
        h.grid = G;
    }
}

// Step 3: the lists the stages behind the front end read.
void plan_lists(const PlanGeom &g, HostPlan &h) {
    if (g.ss) {
        h.tile_utt.resize(h.tiles.size());
        for (int i = 0; i < h.n_utt; i++)
            for (int t = h.uts[i]; t < h.uts[i + 1]; t++) h.tile_utt[t] = i;
    }
    if (g.vad_fused) {
        std::vector<int> &ord = h.vf_order;
        for (int i = 0; i < h.n_utt; i++)
            if (h.frames[i] > 0) ord.push_back(i);
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return h.frames[a] > h.frames[b]; });
        h.n_live = (int)ord.size();
        if (ord.empty()) ord.push_back(0);
    }
    if (g.signal_out) {
        h.out_samples.resize(h.n_utt);
        for (int i = 0; i < h.n_utt; i++) h.out_samples[i] = h.frames[i] * g.wshift + (g.window - g.wshift);
    }
    if (g.chunked && !g.rows_in) {  // the 128-frame chunks: every other 64-frame one
        std::vector<int> &c128 = h.chunks128;
        for (size_t k = 0; k + 1 < h.chunks.size(); k += 2)
            if (!(h.chunks[k + 1] & 64)) {
                c128.push_back(h.chunks[k]);
                c128.push_back(h.chunks[k + 1]);
            }
        h.n_chunks128 = (int)c128.size() / 2;
        if (c128.empty()) c128.assign(2, 0);
    }
}

// Step 4: the scratch of every stage the engine's runs have.  The buffers whose kernels are launched over an empty plan as well -
// the *ss modes' host loop, the fused detector, -remove_dc1, lp_tail_kernel - hold one row at least.
PlanScratch plan_scratch(const PlanGeom &g, const HostPlan &h) {
    const int64_t n = h.n_utt, ro = h.total_frames, n1 = std::max<int64_t>(n, 1), ro1 = std::max<int64_t>(ro, 1);
    PlanScratch s;
    if (g.staged) s.base_rows = ro * g.Dbase;
    if (g.per_utt) s.d_sample_off = n + 1;
    if (g.row_off_dev) s.d_row_off = n + 1;
    if (g.ss) {
        s.ss_seed = s.ss_last = n1 * g.K;
        s.ss_dirty = n1;
        s.ss_vbits = ro1;
    }
    if (g.spectra) s.xri = s.pnr = (g.ss_big ? ro1 : ro) * g.K;
    else if (g.vad_energy) s.pnr = ro;
    if (g.pss) s.pss = ro1 * g.K;
    if (g.vad_burg) s.vad_ci = ro * g.vad_ncoef;
    else if (g.ss_detector) s.vad_ci = ro1 * g.ss_ncep;
    if (g.vad_fused) s.vad_cf = ro1 * VFC_STRIDE;
    if (g.signal_out) s.ybuf = ro * g.window;
    if (g.dc1) s.dc1m = s.dc1 = ro1;
    if (g.logmel) s.logmel = ro * g.B;
    if (g.lp_tail) s.lp_r = (ro1 * (g.lporder + 1) * (g.lags_double ? 8 : 4) + 7) / 8;
    return s;
}
}  // namespace

int build_host_plan(const PlanGeom &g, const int64_t *lengths, int32_t n_utt, HostPlan &out, std::string &err) {
    if (n_utt < 0 || (n_utt && !lengths)) return CTU_ERR_INPUT;
    HostPlan h;
    if (const int rc = plan_layout(g, lengths, n_utt, h, err); rc != CTU_OK) return rc;
    if (g.rows_in) h.grid = std::max(1, std::min(((int)h.tiles.size() + 3) / 4, g.rows_grid_cap));
    else plan_chains(g, h);
    plan_lists(g, h);
    h.scratch = plan_scratch(g, h);
    out = std::move(h);
    return CTU_OK;
}

void vad_ring_step(int32_t order, int64_t frames, int32_t *hidx, int32_t *hsize) {
    // medianFilter::push / flush_frame / cleanFilter as VAD::process_frame, BATCH::flush_vad and VAD::clean drive them over one file
    // (src/vad/vad.h:110-175, src/vad/vad.cc:692-699,705-708,742-745): cleanFilter resets neither historyIdx nor historySize
    if (order < 1 || !hidx || !hsize) return;
    const int delay = (order - 1) / 2;
    int hi = ((*hidx % order) + order) % order, hs = *hsize;
    bool ready = false;
    for (int64_t t = 0; t < frames; t++) {
        hi = (hi + 1) % order;
        if (hs < delay) hs++;
        else ready = true;
    }
    for (;;) {
        if (hs > 0) {
            hi = (hi + 1) % order;
            hs--;
        } else
            ready = false;
        if (!ready) break;
    }
    *hidx = hi;
    *hsize = hs;
}

int64_t vad_ring_rows(int32_t order, int64_t frames, int32_t hidx0, int32_t *src) {
    // the ring of one file: push t writes slot (hidx0 + t) % order; the k-th written row reads slot k % order - at push k + delay, or after
    // the last push for the rows of the flush (src/vad/vad.h:126-175 with `start` reset by cleanFilter, historyIdx not)
    if (order < 1 || frames < 0) return CTU_ERR_INPUT;
    const int delay = (order - 1) / 2;
    if (frames <= delay) return 0;  // the filter never gets ready: nothing is written
    if (!src) return frames;
    const int h0 = ((hidx0 % order) + order) % order;
    std::vector<int32_t> slot((size_t)order, -1);
    int64_t k = 0;
    for (int64_t t = 0; t < frames; t++) {
        slot[(size_t)((h0 + t) % order)] = (int32_t)t;
        if (t >= delay) {
            src[k] = slot[(size_t)(k % order)];
            k++;
        }
    }
    for (; k < frames; k++) src[k] = slot[(size_t)(k % order)];
    return frames;
}

std::vector<int> plan_ring_src(const HostPlan &p, int order, const int32_t *hidx) {
    if (order <= 1) return {};
    bool any = false;
    for (int i = 0; i < p.n_utt; i++) any = any || (hidx[i] % order) != 0;
    if (!any) return {};
    const int delay = (order - 1) / 2;
    std::vector<int> src((size_t)std::max<int64_t>(p.total_frames, 1), -1);
    std::vector<int32_t> rel;
    for (int i = 0; i < p.n_utt; i++) {
        const int64_t T = p.frames[i], r0 = p.row_off[i];
        if (T <= delay) continue;  // nothing is written for it
        rel.assign((size_t)T, -1);
        vad_ring_rows(order, T, hidx[i], rel.data());
        for (int64_t k = 0; k < T; k++) src[(size_t)(r0 + k)] = rel[(size_t)k] < 0 ? -1 : (int)(r0 + rel[(size_t)k]);
    }
    return src;
}

std::vector<int> plan_part_first(const HostPlan &p, int nparts) {
    std::vector<int> first(1, 0);
    const int64_t per = (p.sample_off[p.n_utt] - p.sample_off[0] + nparts - 1) / nparts;
    for (int k = 1; k < nparts; k++) {
        int u = first.back();
        const int64_t goal = p.sample_off[0] + per * k;
        while (u < p.n_utt && p.sample_off[u] < goal) u++;
        if (u > first.back() && u < p.n_utt) first.push_back(u);
    }
    first.push_back(p.n_utt);
    return first;
}

}  // namespace ctu
