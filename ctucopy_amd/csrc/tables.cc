// Which front-end instantiation a configuration runs on and what the kernels' tables hold: host only, HIP-free.  Index arithmetic over
// ctu::Design and the constants of layout_constants.h; the result is one plain value (EngineTables) that engine.hip uploads.
#include "tables.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

namespace ctu {

namespace {

// DCTC: row r of a coefficient table is the value written to output slot r (c1..cN, then c0; norm and lifter are in d.dct):
// the coefficient of every slot (-1: none) and the number of slots written
struct SlotMap {
    std::vector<int> coef_of_slot;
    int nout = 0;
};
SlotMap dct_slots(const Design &d) {
    SlotMap m;
    m.coef_of_slot.assign(d.nfea, -1);
    for (int i = 0; i < d.nfea; i++)
        if (d.row_slot[i] >= 0) {
            m.coef_of_slot[d.row_slot[i]] = i;
            m.nout = std::max(m.nout, d.row_slot[i] + 1);
        }
    return m;
}

// Hann window of the *ss modes' detector, han[i] = 0.5 (1 - cos(2 * 3.141592653 / window * i)) (src/vdet/CepstralDet.h:133-136)
double det_hann(const Design &d, int i) {
    const double m = 2 * 3.141592653 / d.window;
    return 0.5 * (1 - std::cos(m * i));
}
// ... as the 256- / 512-point front end reads it: a sample per lane and register of the detector's 16 lanes, zero beyond the window
void push_det_hann(const Design &d, std::vector<float> &ft) {
    for (int i = 0; i < 16 * (d.wfft == 512 ? VF0_SPL : VF_SPL); i++) ft.push_back(i < d.window ? (float)det_hann(d, i) : 0.f);
}

}  // namespace

Spread spread_small_fft(Design &d) {
    Spread sp;
    sp.user_wfft = d.wfft;
    sp.user_K = d.K;
    if (!(d.wfft < 256 && d.wfft >= 32 && !d.signal_out)) return sp;
    const int S = sp.kstride = 256 / d.wfft;
    for (auto &row : d.fb) {
        std::vector<double> wide(129, 0.0);
        for (int k = 0; k < d.K; k++) wide[(size_t)k * S] = row[k];
        row.swap(wide);
    }
    for (int &f : d.fb_first) f *= S;
    for (int &l : d.fb_last) l *= S;
    d.K = 129;
    d.wfft = 256;
    return sp;
}

void build_phase2(const Design &d, Phase2Tables &t) {
    t.md = md_eligible(d);
    // ---- phase-2 tables.  Bands are dealt to (slot, group) cells: sorted by width, eight per slot, so that the
    // eight lanes of a frame walk bands of similar width in lock step.  A band is cut into 4-bin chunks whose
    // bin range stays inside [0,K); weights outside the band's own [first,last] are zero.
    const int B = d.B;
    std::vector<int> order(B);
    for (int b = 0; b < B; b++) order[b] = b;
    auto width = [&](int b) { return d.fb_last[b] - d.fb_first[b] + 1; };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return width(x) > width(y); });
    const int NS = (B + 7) / 8;
    int ncoef = 0;
    const std::vector<double> *coef_tab = nullptr;
    const bool dctc = d.kind == FeaKind::Dctc && !dct_wide(d);  // (wide: a band-valued front end, no coefficient rows)
    if (dctc) { coef_tab = &d.dct; ncoef = d.nfea; }
    else if (d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa) { coef_tab = &d.idft; ncoef = d.o.fea_lporder + 1; }
    if (ncoef > MAXC) throw std::runtime_error("more cepstral / LP coefficients than the kernel accumulates");
    const int CW = ncoef <= 16 ? 16 : MAXC;  // the kernel has straight-line code for these two widths
    std::vector<int> slot_chunk(NS + 1, 0);
    std::vector<float> cw;                  // chunk weights [NC][8][4]
    std::vector<int> cell(NS * 8 * 2, 0);   // {first bin of the chunk run, band index or -1}
    const int CWS = CW + 4;  // row stride: 20 or 28 floats = 5 or 7 16-byte units, distinct mod 16 over the 8 groups
    std::vector<float> cf((size_t)NS * 8 * CWS, 0.f);
    // LP analysis on uncompressed band energies (no -fb_inld): the same rows in double for the double tail (FEAT_LPD)
    const bool lpd = (d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa) && !d.o.fb_inld;
    std::vector<double> cfd(lpd ? (size_t)NS * 8 * CW : 0, 0.0);
    // DCTC: coefficient row r of a cell is the value written to output slot r
    const SlotMap sm = dctc ? dct_slots(d) : SlotMap();
    const std::vector<int> &coef_of_slot = sm.coef_of_slot;
    t.ncoef_out = sm.nout;
    auto chunks_of = [&](int b) {  // chunks of 4 bins from the aligned start of the band to its last bin
        const int k0 = d.fb_first[b] & ~3;
        return (d.fb_last[b] - k0) / 4 + 1;
    };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return chunks_of(x) > chunks_of(y); });
    for (int sl = 0; sl < NS; sl++) {
        int nch = 0;
        for (int g = 0; g < 8 && sl * 8 + g < B; g++) nch = std::max(nch, chunks_of(order[sl * 8 + g]));
        if (4 * nch > PSTRIDE) throw std::runtime_error("filter band wider than the spectrum");
        slot_chunk[sl] = (int)cw.size() / 32;
        // Phase 2 reads P with one ds_read_b128 per lane; the 16-byte unit a lane touches is
        // (frame + kstart/4 + chunk) mod 16 (rows are 65 units apart).  A b128 wave access is served in four groups of
        // 16 lanes = {frame f: groups 0-3, f+1: groups 4-7, f+2: groups 4-7, f+3: groups 0-3}; collisions depend only
        // on a_g = kstart_g/4.  Search the assignment of this slot's bands to groups (and up to `slack` leading
        // zero chunks) for the fewest colliding lane pairs.
        std::vector<int> perm(8), best_perm(8), lead(8, 0), best_lead(8, 0);
        for (int g = 0; g < 8; g++) perm[g] = best_perm[g] = sl * 8 + g < B ? order[sl * 8 + g] : -1;
        auto a_of = [&](int b, int ld) { return b < 0 ? -1000 : (std::min(d.fb_first[b] & ~3, PSTRIDE - 4 * nch) / 4 - ld); };
        auto cost = [&](const std::vector<int> &pm, const std::vector<int> &ld) {
            int c = 0, a[8];
            for (int g = 0; g < 8; g++) a[g] = a_of(pm[g], ld[g]);
            // a ds_read_b128 is served in four groups of 16 lanes: {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32
            static const int grp[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                           {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
            for (int q = 0; q < 4; q++) {
                int unit[16];
                for (int i = 0; i < 16; i++) {
                    const int lane = grp[q & 1][i] + 32 * (q >> 1);
                    const int f8 = t.md ? (lane & 7) : (lane >> 3), g = t.md ? (((lane >> 3) & 1) * 4 + (lane >> 4)) : (lane & 7);
                    unit[i] = a[g] < -500 ? -1 - i : ((a[g] + f8) % 16 + 16) % 16;  // rows are 65 units apart
                }
                for (int i = 0; i < 16; i++)
                    for (int j = i + 1; j < 16; j++) c += (unit[i] >= 0 && unit[i] == unit[j]);
            }
            return c;
        };
        {
            int best = cost(perm, lead);
            uint32_t rng = 12345u + sl;
            for (int it = 0; it < 4000 && best > 0; it++) {
                std::vector<int> pm = best_perm, ld = best_lead;
                rng = rng * 1664525u + 1013904223u;
                const int i = (rng >> 8) % 8, j = (rng >> 16) % 8;
                std::swap(pm[i], pm[j]);
                std::swap(ld[i], ld[j]);
                rng = rng * 1664525u + 1013904223u;
                const int g = (rng >> 8) % 8;
                if (pm[g] >= 0) {
                    // leading zero chunks are allowed while the run still starts at >= 0 and ends beyond the last bin
                    const int k0 = std::min(d.fb_first[pm[g]] & ~3, PSTRIDE - 4 * nch);
                    const int mx = std::min({3, k0 / 4, (k0 + 4 * nch - (d.fb_last[pm[g]] + 1)) / 4});
                    ld[g] = mx > 0 ? (int)((rng >> 20) % (mx + 1)) : 0;
                }
                const int c = cost(pm, ld);
                if (c <= best) {
                    best = c;
                    best_perm = pm;
                    best_lead = ld;
                }
            }
        }
        std::vector<int> kstart(8, 0);
        for (int g = 0; g < 8; g++) {
            cell[(sl * 8 + g) * 2 + 1] = -1;
            if (best_perm[g] < 0) continue;
            const int b = best_perm[g];
            // aligned start; the run of nch chunks must end inside the row's PSTRIDE floats (bins >= K get weight 0
            // but are read, so the kernel keeps them finite: it zeroes the row padding once per workgroup)
            kstart[g] = std::min(d.fb_first[b] & ~3, PSTRIDE - 4 * nch) - 4 * best_lead[g];
            cell[(sl * 8 + g) * 2] = kstart[g];
            cell[(sl * 8 + g) * 2 + 1] = b;
            for (int i = 0; i < ncoef; i++) {
                const int src = dctc ? coef_of_slot[i] : i;
                if (src >= 0) cf[((size_t)sl * 8 + g) * CWS + i] = (float)(*coef_tab)[(size_t)src * B + b];
                if (src >= 0 && lpd) cfd[((size_t)sl * 8 + g) * CW + i] = (*coef_tab)[(size_t)src * B + b];
            }
        }
        for (int ch = 0; ch < nch; ch++)
            for (int g = 0; g < 8; g++)
                for (int i = 0; i < 4; i++) {
                    float w = 0.f;
                    if (best_perm[g] >= 0) {
                        const int b = best_perm[g], k = kstart[g] + 4 * ch + i;
                        if (k >= d.fb_first[b] && k <= d.fb_last[b]) w = (float)d.fb[b][k];
                    }
                    cw.push_back(w);
                }
    }
    slot_chunk[NS] = (int)cw.size() / 32;
    std::vector<float> ft(cw);
    t.cells = cell;
    t.slot_chunk = slot_chunk;
    auto push_ints = [&](const std::vector<int> &v) {
        for (int x : v) {
            float f;
            std::memcpy(&f, &x, 4);
            ft.push_back(f);
        }
        while (ft.size() & 3) ft.push_back(0.f);
    };
    t.ck_off = (int)ft.size();
    {   // the kernel's records: {first bin, band or -1, first chunk of the slot, chunks of the slot}; one more slot of idle cells, which
        // the walk prefetches behind the last one
        std::vector<int> rec4((size_t)(NS + 1) * 8 * 4, 0);
        for (int sl = 0; sl <= NS; sl++)
            for (int g = 0; g < 8; g++) {
                int *r = &rec4[(size_t)(sl * 8 + g) * 4];
                r[0] = sl < NS ? cell[(sl * 8 + g) * 2] : 0;
                r[1] = sl < NS ? cell[(sl * 8 + g) * 2 + 1] : -1;
                r[2] = slot_chunk[std::min(sl, NS)];
                r[3] = sl < NS ? slot_chunk[sl + 1] - slot_chunk[sl] : 0;
            }
        push_ints(rec4);
    }
    t.cf_off = (int)ft.size();
    if (!t.md) ft.insert(ft.end(), cf.begin(), cf.end());  // the MFMA tail reads the am table below instead
    while (ft.size() & 3) ft.push_back(0.f);
    if (t.md) {
        // A operands of the DCT MFMAs: for slot sl and half h, lane m + 16 kk holds row m of the folded DCT table (LP chain: of
        // the cosine iDFT table) at the band of cell (sl, group kk + 4 h); zero for idle cells and for rows >= the number of output slots
        t.am_off = (int)ft.size();
        for (int sl = 0; sl < NS; sl++)
            for (int h = 0; h < 2; h++)
                for (int lane = 0; lane < 64; lane++) {
                    const int m = lane & 15, g = (lane >> 4) + 4 * h;
                    const int b = cell[(sl * 8 + g) * 2 + 1];
                    float v = 0.f;
                    if (dctc) {
                        if (b >= 0 && m < t.ncoef_out && coef_of_slot[m] >= 0) v = (float)(*coef_tab)[(size_t)coef_of_slot[m] * B + b];
                    } else if (b >= 0 && m < ncoef) v = (float)(*coef_tab)[(size_t)m * B + b];  // LP: row m = lag m
                    ft.push_back(v);
                }
    }
    if (lpd) {
        t.cfd_off = (int)ft.size();  // a multiple of 4 floats: 8-byte aligned in LDS
        for (double v : cfd) {
            float h[2];
            std::memcpy(h, &v, 8);
            ft.push_back(h[0]);
            ft.push_back(h[1]);
        }
        while (ft.size() & 3) ft.push_back(0.f);
    }
    if (ss_eligible(d)) {
        t.han_off = (int)ft.size();
        push_det_hann(d, ft);
    }
    t.tab_floats = (int)ft.size();
    t.NS = NS;
    t.CW = CW;
    t.lift_off = (int)ft.size();
    for (double v : d.lifter) ft.push_back((float)v);
    ft.push_back(0.f);
    t.ft = ft;
    std::vector<int> it(slot_chunk);
    it.insert(it.end(), d.row_slot.begin(), d.row_slot.end());
    t.it = it;
}

// Rebuilds every band's dense weight row from the chunk tables and returns the largest deviation from the
// float-rounded filter bank (0 when the tables are consistent).
double check_phase2(const Design &d, const Phase2Tables &t) {
    double worst = 0;
    std::vector<int> seen(d.B, 0);
    for (int sl = 0; sl < t.NS; sl++)
        for (int g = 0; g < 8; g++) {
            const int kstart = t.cells[(sl * 8 + g) * 2], b = t.cells[(sl * 8 + g) * 2 + 1];
            if (b < 0) continue;
            seen[b]++;
            std::vector<double> row(PSTRIDE, 0.0);
            for (int ch = t.slot_chunk[sl]; ch < t.slot_chunk[sl + 1]; ch++)
                for (int i = 0; i < 4; i++) {
                    const int k = kstart + 4 * (ch - t.slot_chunk[sl]) + i;
                    if (k < 0 || k >= PSTRIDE) return 1e30;
                    row[k] += t.ft[(size_t)(ch * 8 + g) * 4 + i];
                }
            for (int k = 0; k < PSTRIDE; k++) {
                const double want = (k < d.K && k >= d.fb_first[b] && k <= d.fb_last[b]) ? (double)(float)d.fb[b][k] : 0.0;
                if (std::fabs(row[k] - want) > 0 && getenv("CTU_P2_DEBUG")) fprintf(stderr, "sl %d g %d band %d k %d kstart %d first %d last %d row %g want %g nch %d\n", sl, g, b, k, kstart, d.fb_first[b], d.fb_last[b], row[k], want, t.slot_chunk[sl+1]-t.slot_chunk[sl]);
                worst = std::max(worst, std::fabs(row[k] - want));
            }
        }
    for (int b = 0; b < d.B; b++)
        if (seen[b] != 1) return 1e30;
    return worst;
}

// The compiled walk signature (phase2_walks.h) that this bank matches, or -1: the chunk counts per slot must be the entry's and the
// frames the shape the entries are compiled for.  The one place that compares banks; fe_select uses the match where the
// instantiation it chose is the one the entry was compiled with, every other instantiation walks generically.  A
// straight-line walk is correct for every bank with these counts (first bins and band indices stay per-lane records).
int match_walk(const Design &d, const std::vector<int> &slot_chunk) {
    if (d.wfft != WALK_WFFT || (d.window + 31) / 32 != WALK_NZ) return -1;
    int found = -1;
    for_each_walk([&](auto w) {
        typedef decltype(w) W;
        if (found >= 0 || (int)slot_chunk.size() != W::NS + 1) return;
        for (int s = 0; s <= W::NS; s++)
            if (slot_chunk[s] != W::first(s)) return;
        found = W::index;
    });
    return found;
}

// The name that keys the profiles: the walk, the export and the row width are not shown.
std::string fe_name(const FeSel &k) {
    const char *feat = k.feat == FEAT_DCTC ? "DCTC" : k.feat == FEAT_BANDS ? "BANDS" : k.feat == FEAT_LP ? "LP" : "LPD";
    const char *gen = k.gen == GEN_PLAIN ? "plain" : k.gen == GEN_INLD ? "inld" : k.gen == GEN_EXTEN ? "exten" : "full";
    return "frontend_kernel<" + std::to_string(k.nz) + ", " + feat + ", MODE " + std::to_string(k.mode) + ", " + gen + (k.md ? ", MD" : "") + (k.vf ? ", VF" : "") +
           (k.ss ? ", SS" : "") + (k.sy ? ", SY" : "") + ">";
}

// The instantiation a configuration runs on, from the design (after ctu_engine_create has spread an FFT size below 256 onto the 256-point
// mode) and its phase-2 tables (`t`; none with speech output).  Needs no device.  Specialised instantiations (see GEN in
// frontend_kernel.h): the plain chain, plain + intensity-loudness law for the 16-coefficient LP path (PLP), plain + exten for
// 16-coefficient DCT / band outputs; the cepstral ones of these run their DCT tail on the matrix cores (MD, tables laid out for it by
// build_phase2).  Everything else, and every run with the VAD export, reads its flags at run time.
FeSel fe_select(const Design &d, const Phase2Tables *t) {
    const Opts &o = d.o;
    FeSel k;
    if (d.wfft >= 1024) return k;
    const bool signal = d.signal_out, exten = o.nr_mode == "exten";
    // ---- what the configuration and its tables fix
    k.mode = d.wfft == 256;
    k.sy = signal;
    k.ss = ss_eligible(d);
    k.vf = !signal && vf_eligible(d);
    k.md = t && t->md;             // the tables are laid out for the MFMA tail's lane map
    k.nc = t ? t->CW : 16;         // rows of MAXC entries: more than 16 cepstra / LP lags
    if (signal || dct_wide(d) || (d.kind != FeaKind::Dctc && d.kind != FeaKind::Lpc && d.kind != FeaKind::Lpa)) k.feat = FEAT_BANDS;
    else k.feat = d.kind == FeaKind::Dctc ? FEAT_DCTC : o.fb_inld ? FEAT_LP : FEAT_LPD;
    // rows of samples per lane that can be non-zero.  The 13-row instantiations serve the 25 ms windows (the *ss modes: every window of
    // at most 13 rows - the window table is zero beyond the window); every other window, and -remove_dc1, takes the generic row count
    const int rows = k.mode ? (d.window + 15) / 16 : (d.window + 31) / 32;
    k.nz = (!o.remove_dc1 && (rows == 13 || (k.ss && rows < 13))) ? 13 : 16;
    // the spectra leave the kernel for the VAD kernels (Burg-cepstral and energy criteria)
    k.vx = o.do_vad() && !k.vf && !signal && (o.vad_cri_mode == "energy" || o.vad_cepdist_mode == "lpc");
    bool diag = false;
#ifdef CTU_DIAG  // phase ablation (ctu_engine_run: kp.dbg) is a run-time flag
    diag = getenv("CTU_DEBUG_MODE") && atoi(getenv("CTU_DEBUG_MODE")) != 0;
#endif
    // the plain chain: every flag a specialised GEN turns into a constant has its default
    const bool base = !k.vx && !o.fea_E && o.fb_power && o.remove_dc && !o.remove_dc1 && !diag && !signal && !o.nr_when_afterFB;
    const bool lp12 = o.fea_lporder == 12 && o.fea_ncepcoefs == 12 && d.kind != FeaKind::Lpa;  // the PLP preset exactly: order and number of cepstra fixed at compile time (LPO)
    // ---- GEN and LPO, top to bottom
    k.gen = GEN_FULL;
    if (o.remove_dc1) k.gen = GEN_DC1;  // no spectrum export
    else if (k.sy) {}                   // speech output: no phase 2, the flags at run time
    else if (k.ss) {
        // the straight-line lattices name the window's last sample: the presets' windows, cepstra on the matrix cores or plain band outputs.
        // Energy columns, -fb_inld, -fb_power off, the LP kinds, other windows: the flags at run time
        const bool preset_win = d.window == (k.mode ? VF_WINDOW : VF0_WINDOW);
        if (preset_win && ((k.md && k.feat == FEAT_DCTC) || (k.feat == FEAT_BANDS && base && !o.fb_inld))) {
            k.gen = GEN_PLAIN;
            k.lpo = o.fea_ncepcoefs == 12 ? 12 : 0;  // the detector's order is -fea_ncepcoefs
        }
    }
    else if (k.vf) k.gen = exten ? GEN_EXTEN : GEN_PLAIN;
    else if (k.md && k.feat == FEAT_LP) {  // the compressed-band LP chain: lags by the MFMA tail, the recursions in lp_tail_kernel
        k.gen = GEN_INLD;
        k.lpo = lp12 ? 12 : 0;
    }
    else if (k.md) k.gen = exten ? GEN_EXTEN : GEN_PLAIN;
    else if (k.vx) {}
    else if (base && !o.fb_inld && !exten && k.feat != FEAT_LPD) k.gen = GEN_PLAIN;
    else if (base && o.fb_inld && !exten && k.nc == 16 && k.feat == FEAT_LP) {
        k.gen = GEN_INLD;
        k.lpo = lp12 ? 12 : 0;
    }
    else if (base && !o.fb_inld && exten && k.feat == FEAT_BANDS) k.gen = GEN_EXTEN;
    // ---- the straight-line filter-bank walk, where the bank matches the entry compiled for exactly this instantiation
    if (t) {  // CTU_PHASE2_GENERIC=1: the generic walk for every bank (A/B and identity checks inside one build)
        const char *g = getenv("CTU_PHASE2_GENERIC");
        const int m = (g && atoi(g) != 0) ? -1 : match_walk(d, t->slot_chunk);
        for_each_walk([&](auto w) {
            if (m == w.index && walk_serves<decltype(w)>(k)) k.walk = m;
        });
    }
    // what the eligibility rules (md_eligible, vf_eligible, ss_eligible) promise the tree above: the instantiation exists, and a specialised
    // GEN's constants are the configuration's flags
    const bool flags_ok = k.gen == GEN_FULL || k.gen == GEN_DC1 || (base && o.fb_inld == (k.gen == GEN_INLD) && exten == (k.gen == GEN_EXTEN));
    if (!fe_compiled(k) || !flags_ok) throw std::runtime_error("internal: no front-end instantiation for this configuration (" + fe_name(k) + ")");
    return k;
}

namespace {

// TRAP-DCT: the folded table and, where trapdct_split16_kernel serves the shape, its
// A operands: G shifted by the frame phase c, zero-padded to 128 taps, each value split into two
// fp16 terms (round to nearest even at every step, as the device splits the data)
void build_trap(const Design &d, EngineTables &e) {
    e.trapG.assign(d.trap.begin(), d.trap.end());
    const int tl = d.o.fea_trapdct_traplen, nd = d.o.fea_trapdct_ndct, half = (tl - 1) / 2;
    e.trap_bf16 = trap_path(d.B, tl, nd).split16 != 0;  // (layout_constants.h: the one statement of which kernel runs)
    if (!e.trap_bf16) return;
    const int NT = 2;
    e.trapG16.assign((size_t)8 * 4 * NT * 64 * 4, 0u);  // records of four words
    for (int c = 0; c < 8; c++)
        for (int s_ = 0; s_ < 4; s_++)
            for (int lane = 0; lane < 64; lane++) {
                const int m = lane & 15, q = lane >> 4;
                uint16_t term[NT][8];
                for (int i = 0; i < 8; i++) {
                    const int j = 32 * s_ + 8 * q + i - c - (TB_OFF - half);
                    const float v = (m < nd && j >= 0 && j < tl) ? (float)d.trap[(size_t)m * tl + j] : 0.f;
                    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
                    std::memcpy(&term[0][i], &h, 2);
                    std::memcpy(&term[1][i], &l, 2);
                }
                for (int sp = 0; sp < NT; sp++) {
                    uint32_t *w = &e.trapG16[((((size_t)c * 4 + s_) * NT + sp) * 64 + lane) * 4];
                    for (int i = 0; i < 4; i++) w[i] = term[sp][2 * i] | ((uint32_t)term[sp][2 * i + 1] << 16);
                }
            }
}

// The tables of the large-FFT kernels (bigfft_kernel.h, wave1k_kernel.h)
void build_big_tables(const Design &d, EngineTables &e) {
    const double pi = 3.14159265358979323846;
    e.big_win.assign(d.hamming.begin(), d.hamming.end());
    e.big_tw.resize((size_t)d.wfft / 2 * 2);
    for (int m = 0; m < d.wfft / 2; m++) {
        const double a = 2.0 * pi * (double)m / (double)d.wfft;
        e.big_tw[2 * (size_t)m] = (float)std::cos(a);
        e.big_tw[2 * (size_t)m + 1] = (float)-std::sin(a);
    }
    std::vector<float> &fbw = e.big_fbw;
    std::vector<int> &range = e.big_range, &seg = e.big_seg, &slot = e.big_slot;
    range.assign((size_t)d.B * 3, 0);
    for (int b = 0; b < d.B; b++) {
        range[3 * b] = d.fb_first[b];
        range[3 * b + 1] = d.fb_last[b];
        range[3 * b + 2] = (int)fbw.size();
        for (int k = d.fb_first[b]; k <= d.fb_last[b]; k++) fbw.push_back((float)d.fb[b][k]);
    }
    e.big_fb_total = (int)fbw.size();
    if (fbw.empty()) fbw.push_back(0.f);
    {
        // wave1k_kernel's bank: the bands' bin runs cut into at most 64 segments of at most S bins (the smallest S that fits)
        seg.assign(256 + 2 * (size_t)std::max(d.B, 1), 0);
        if (d.B <= 64) {
            int S = 1;
            for (;; S++) {
                int n = 0;
                for (int b = 0; b < d.B; b++) n += std::max(1, (d.fb_last[b] - d.fb_first[b] + 1 + S - 1) / S);
                if (n <= 64) break;
            }
            int lane = 0;
            for (int b = 0; b < d.B; b++) {
                const int w = d.fb_last[b] - d.fb_first[b] + 1, ns = std::max(1, (w + S - 1) / S);
                seg[256 + 2 * b] = lane;
                seg[256 + 2 * b + 1] = ns;
                for (int i = 0; i < ns; i++, lane++) {
                    const int k0 = d.fb_first[b] + i * S, cnt = std::max(0, std::min(S, w - i * S));
                    seg[4 * lane] = b;
                    seg[4 * lane + 1] = k0;
                    seg[4 * lane + 2] = cnt;
                    seg[4 * lane + 3] = range[3 * b + 2] + i * S;
                }
            }
        }
    }
    std::vector<float> &coef = e.big_coef;
    coef.assign(4, 0.f);
    e.big_coef_d.assign(4, 0.0);
    slot.assign(4, -1);
    const bool wide = dct_wide(d);  // a band-valued front end, no coefficient rows
    if (d.kind == FeaKind::Dctc && !wide) {
        const SlotMap sm = dct_slots(d);
        const std::vector<int> &coef_of_slot = sm.coef_of_slot;
        const int nout = e.p2.ncoef_out = sm.nout;
        coef.assign((size_t)std::max(nout, 1) * d.B, 0.f);
        slot.assign(std::max(nout, 1), -1);
        for (int r = 0; r < nout; r++) {
            slot[r] = coef_of_slot[r];
            if (coef_of_slot[r] >= 0)
                for (int b = 0; b < d.B; b++) coef[(size_t)r * d.B + b] = (float)d.dct[(size_t)coef_of_slot[r] * d.B + b];
        }
    } else if (d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa) {
        e.big_coef_d.assign(d.idft.begin(), d.idft.end());
        slot.assign(d.row_slot.begin(), d.row_slot.end());
        while (slot.size() < (size_t)MAX_LP + 2) slot.push_back(-1);
    }
    e.big_lifter.assign(d.lifter.begin(), d.lifter.end());
    e.big_lifter.push_back(0.f);
    e.lanec.assign(16 * LANEC, 0.f);  // the tables of the 512 / 256-point kernels stay empty (e.p2)
    switch (d.kind) {
        case FeaKind::Dctc: e.feat = wide ? FEAT_BANDS : FEAT_DCTC; break;
        case FeaKind::Lpc:
        case FeaKind::Lpa: e.feat = FEAT_LP; break;
        default: e.feat = FEAT_BANDS; break;
    }
}

// A operands of dct_wide_kernel (dctw_kernel.h): [chunk][row block][k-step][lane], lane m + 16 k holding row m of the block at band
// 64 chunk + 4 step + k.  Row r of the table is the value written to row column r.
void build_dctw(const Design &d, EngineTables &e) {
    const SlotMap sm = dct_slots(d);
    const std::vector<int> &coef_of_slot = sm.coef_of_slot;
    const int nout = sm.nout;
    if (nout <= 16 || nout > DCTW_MAX) throw std::runtime_error("internal: row width outside dct_wide_kernel's row blocks");
    const int nrb = (nout + 15) / 16, chunks = (d.B + DCTW_KC - 1) / DCTW_KC, KS = DCTW_KC / 4;
    std::vector<float> &tab = e.dctw_tab;
    tab.assign((size_t)chunks * nrb * KS * 64, 0.f);
    for (int c = 0; c < chunks; c++)
        for (int rb = 0; rb < nrb; rb++)
            for (int s_ = 0; s_ < KS; s_++)
                for (int lane = 0; lane < 64; lane++) {
                    const int r = rb * 16 + (lane & 15), b = c * DCTW_KC + 4 * s_ + (lane >> 4);
                    if (r < nout && b < d.B && coef_of_slot[r] >= 0)
                        tab[(((size_t)c * nrb + rb) * KS + s_) * 64 + lane] = (float)d.dct[(size_t)coef_of_slot[r] * d.B + b];
                }
    e.dctw_nout = nout;
    e.dctw_chunks = chunks;
}

}  // namespace

EngineTables build_engine_tables(const Design &d) {
    EngineTables e;
    const double pi = 3.14159265358979323846;
    e.big = d.wfft >= 1024;
    e.dctw = dct_wide(d);
    if (e.dctw) build_dctw(d, e);
    if (d.kind == FeaKind::TrapDct) build_trap(d, e);
    if (e.big) {
        // (-remove_dc1 at 1024 points takes bigfft_kernel<4>, which reads the frames' offsets)
        // (and speech output and the Burg-cepstral VAD criterion: the spectra's export is bigfft_kernel's)
        const bool burg = d.o.do_vad() && d.o.vad_cri_mode == "cepdist" && d.o.vad_cepdist_mode == "lpc";
        const bool wave1k = d.wfft == 1024 && !d.o.remove_dc1 && !d.signal_out && !burg && !(getenv("CTU_WAVE1K") && atoi(getenv("CTU_WAVE1K")) == 0);
        build_big_tables(d, e);
        e.ss = ss_big_eligible(d) ? ss_mode_of(d.o) : 0;
        e.ss_file = e.ss && d.o.vadmode == "file";
        e.path = wave1k ? BIG_WAVE1K : e.ss ? BIG_SS : BIG_FFT;
        if (e.ss && !e.ss_file)
            for (int i = 0; i < d.window; i++) e.big_han.push_back(det_hann(d, i));
        return e;
    }
    // ---- the 512 / 256-point front end: the phase-2 tables (none with speech output), then the instantiation, then what follows from it
    Phase2Tables &t = e.p2;
    if (!d.signal_out) {
        build_phase2(d, t);
        if (check_phase2(d, t) != 0.0) throw std::runtime_error("internal: phase-2 chunk tables do not reproduce the filter bank");
    }
    const FeSel k = e.sel = fe_select(d, d.signal_out ? nullptr : &t);
    e.feat = k.feat;
    e.ss = k.ss ? ss_mode_of(d.o) : 0;
    e.ss_file = e.ss && d.o.vadmode == "file";
    // The DUAL instantiations (frontend_kernel.h: the plain chain, with or without the intensity-loudness law) take their window scaled by 1/2: the packed transform's untangle owes the
    // power spectrum a factor 1/4, and a power of two on the window goes through every rounding of the chain unchanged - the rows are
    // bit for bit those of 0.25f * (re^2 + im^2), two multiplications per bin pair cheaper.
    const float wscale = fe_dual(k.nz, k.mode, k.vx, k.gen, k.vf, k.ss, k.sy) ? 0.5f : 1.f;
    // ---- per-lane constant records (see LC_* in layout_constants.h)
    const bool mode1 = k.mode == 1;
    std::vector<float> &lc = e.lanec;
    lc.assign(16 * LANEC, 0.f);
    for (int l = 0; l < 16; l++) {
        float *r = lc.data() + l * LANEC;
        for (int j = 0; j < 16; j++)
            for (int h = 0; h < 2; h++) {
                // MODE 0: lane l holds samples 32j+2l, +1 of row j; MODE 1: sample 16j+l (second slot unused)
                const int i = mode1 ? (h ? d.window : 16 * j + l) : 32 * j + 2 * l + h;
                r[LC_WIN + 2 * j + h] = i < d.window ? (float)d.hamming[i] * wscale : 0.f;
                r[LC_MASK + 2 * j + h] = i < d.window ? 1.f : 0.f;
            }
        for (int k1 = 1; k1 < 16; k1++) {
            const double a = -2 * pi * (double)(k1 * l) / 256.0;
            r[LC_TW + 2 * (k1 - 1)] = (float)std::cos(a);
            r[LC_TW + 2 * (k1 - 1) + 1] = (float)std::sin(a);
        }
        for (int k2 = 0; k2 < 8; k2++) {
            const double a = -2 * pi * (double)(l + 16 * k2) / 512.0;
            r[LC_UT + 2 * k2] = (float)std::cos(a);
            r[LC_UT + 2 * k2 + 1] = (float)std::sin(a);
        }
    }
    if (d.signal_out) {  // nothing is projected: the empty table area
        t.CW = 16;
        if (e.ss) {  // the detector's Hann window is the only table (as build_phase2 lays it out for the feature path)
            t.ft.clear();
            push_det_hann(d, t.ft);
            t.tab_floats = t.lift_off = (int)t.ft.size();
            t.ft.push_back(0.f);  // (where the lifter sits on the feature path)
        }
    }
    e.lds_bytes = ((size_t)TILE * PSTRIDE + t.tab_floats + LTW_FLOATS + (d.o.nr_when_afterFB ? NWAVE * 128 : 0) +
                   ((k.vf || k.ss) && !k.mode ? NWAVE * VF0_STAGE : 0)) * sizeof(float);  // 512-point detector paths: staged frames per wave
    if (e.lds_bytes > 160 * 1024) throw std::runtime_error("configuration needs more than 160 KiB of LDS");
    return e;
}

std::vector<double> host_tables_report(Design &d) {
    const Spread sp = spread_small_fft(d);
    const EngineTables e = build_engine_tables(d);
    const VadParams vp = vad_params(d, sp);
    const FeSel &k = e.sel;
    const Phase2Tables &t = e.p2;
    std::vector<double> v = {(double)k.nz, (double)k.feat, (double)k.mode, (double)k.vx, (double)k.nc, (double)k.gen, (double)k.lpo, (double)k.md,
                             (double)k.vf, (double)k.ss, (double)k.sy, (double)k.walk,
                             (double)e.feat, (double)e.big, (double)e.path, (double)e.ss, (double)e.ss_file, (double)e.dctw, (double)e.trap_bf16,
                             (double)e.lds_bytes, (double)e.dctw_nout, (double)e.dctw_chunks, (double)e.big_fb_total,
                             (double)t.lift_off, (double)t.tab_floats, (double)t.ck_off, (double)t.cf_off, (double)t.cfd_off, (double)t.am_off,
                             (double)t.han_off, (double)t.NS, (double)t.CW, (double)t.ncoef_out, (double)sp.kstride, (double)sp.user_wfft, (double)sp.user_K};
    auto image = [&](const auto &tab) {  // the length in 32-bit words, then the words
        typedef typename std::decay<decltype(tab)>::type::value_type T;
        const size_t words = tab.size() * sizeof(T) / 4;
        v.push_back((double)words);
        for (size_t i = 0; i < words; i++) {
            uint32_t w;
            std::memcpy(&w, reinterpret_cast<const char *>(tab.data()) + 4 * i, 4);
            v.push_back((double)w);
        }
    };
    image(e.lanec); image(t.ft); image(t.it); image(e.trapG); image(e.trapG16); image(e.dctw_tab);
    image(e.big_win); image(e.big_tw); image(e.big_fbw); image(e.big_range); image(e.big_seg); image(e.big_coef); image(e.big_coef_d);
    image(e.big_slot); image(e.big_lifter); image(e.big_han);
    for (double x : {(double)vp.K, (double)vp.wfft, (double)vp.window, (double)vp.ncoef, (double)vp.krow, (double)vp.kstride, (double)vp.cri, (double)vp.thr,
                     (double)vp.energy_db, (double)vp.cep_init, (double)vp.filter_order, vp.cep_p, vp.abs_thr, vp.perc_thr, vp.adapt_q, vp.adapt_za,
                     vp.dyn_perc, vp.dyn_min, vp.qmaxinc, vp.qmaxdec, vp.qmindec, vp.qmininc, (double)vp.perc_init, (double)vp.adapt_init,
                     (double)vp.dyn_init, (double)vp.D, (double)vp.ncep, (double)vp.c0_slot, (double)vp.fea_blk, (double)vp.delay, (double)vp.e_slot,
                     (double)vp.e_delay})
        v.push_back(x);
    return v;
}

}  // namespace ctu
