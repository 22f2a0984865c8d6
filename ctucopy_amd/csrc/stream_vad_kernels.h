// Streaming input with detector state (include/ctu_engine.h: CTU_STREAMS_VAD_STATE): the VAD module's sequential part on the frames of a
// push.  Included by engine.hip behind vad_kernels.h and stream_rows_kernels.h, whose recurrences and row arithmetic these kernels use.
//
// The front end of a push and the criterion kernels behind it (vad_a2c_kernel, vad_burg_kernel, the energy export) are the offline ones:
// they are frame-parallel and leave the criterion's input of every frame of the push in the plan's scratch, by the push's dense row
// index.  What runs along a file is the replay - cepstral distance to the adaptive background, the threshold recurrences, the
// background's update, the majority filter (vad_kernels.h: VadRun, vad_frame, vad_lanes_kernel) - and all of it is causal: frame t reads
// the state frames 0 .. t - 1 left.  So the replay of a push starts from the state the stream's last push stored and stores it again
// behind its last frame.  Every branch of the recurrences that names a frame (t == 0, t == 1, perc_init, adapt_init, dyn_init, cep_init,
// the filter's t >= h) takes the ABSOLUTE frame index t = F0 + i, with F0 the host's mirror of the file's frames ahead of the push
// (RowPush::F0), never the index within the push.  A file's first push (F0 == 0) starts from the zero state and loads nothing, so neither
// create nor finish clears device state.
//
// The majority filter releases a decision h = (filter_order - 1) / 2 frames late and the reference's writer releases the row with it
// (src/vad/vad.h:126-175, src/io/batch.cc:230-249): frame t >= h emits the byte of row t - h.  After F frames R(F) = max(F - h, 0)
// bytes are out, which is stream_rows_out(h, h - 1, F): the RowPush descriptors of stream_rows_kernels.h carry rows and bytes alike
// (byte k of a push belongs to row k of the same push: out0 serves both), the two histories per stream keep the last h base rows, and
// stream_rows_carry_kernel moves them.  Nothing counts on the device: where a byte goes is r0 = R(F0) of the host.
//
//   stream_vad_lanes_kernel<NCL, THR>  the fused criterion's replay (vad_quad_step, which vad_lanes_kernel calls too): 16 pushed streams per
//                                      wave, four lanes each
//   stream_vad_decide_kernel           the energy and the non-fused Burg criterion: VadRun + vad_frame as they stand, a wave per pushed
//                                      stream.  Coverage, not a tuned path: 64 lanes do one stream's scalar work
//   stream_vad_rows_kernel             rows r0 .. r0 + nr - 1 of every pushed stream, copied h frames late (stream_base_row's two sources)
//   stream_vad_finish_kernel           the end of a file: vad_flush's zeros through the filter, the last min(F, h) bytes and rows
//
// Behind row state (CTU_STREAMS_VAD_ROW_STATE beside the two: a delta chain, a stacking or CMS behind the detector) the reference calls the
// detector when a vector reaches the writer (src/io/batch.cc:172-192,230-241,251-291): call j - the index every branch of the recurrences
// takes - reads the criterion of frame min(j + delay, T - 1), delay the chain's halo H.  After F frames C(F) = stream_rows_out(H, wmax, F)
// calls are made and R(F) = max(C(F) - h, 0) rows and bytes are out; the host says which calls a push makes (VadCalls, stream_plan.h).  Once
// F >= wmax + 2 the calls of a push read the push's own frames; the push in which F crosses wmax + 2 may read frame F0 - 1 (a stacking,
// H = wmax, with the boundary between frames wmax and wmax + 1), and the end of a file repeats frame T - 1's criterion for the calls
// C(T) .. T - 1.  Both are served by one record per stream, in a buffer of its own (crec: the newest frame's criterion input, one energy or
// ncoef <= 32 Burg cepstra, doubles stored and reloaded as they stand); vstate and the fused kernel's layout are untouched - the fused
// criterion only ever runs here with delay 0, as it stands.  The rows are the row kernels' (stream_rows_kernels.h), over histories h rows deeper.
//   stream_vad_delayed_kernel          stream_vad_decide_kernel's twin: the calls of a push, then the push's newest frame into the record
//   stream_vad_delayed_finish_kernel   stream_vad_finish_kernel's twin: the calls the file still owes on the record, then vad_flush
//
// State (vstate): one record of VST_DOUBLES doubles per stream, 384 bytes, 128-byte aligned when the array is:
//   [0..6]   crimin, crimax, crimean, crimean2, crivar, dmin, dmax          (VadThr's seven doubles)
//   [7]      hist: the majority filter's ring of raw decisions, bit k = slot k   (64 bits, stored as they stand)
//   [8]      adapt_vad (low word) | hidx (high word)
//   [9]      nsum (low word) | spare.  VadRun::nout, the fourth int, is not kept: it is R(F0), which the host mirrors
//   [10..15] spare
//   [16..47] c0: the background cepstrum, coefficient k at [16 + k] (32 at most; the fused path's 14 in the first 16)
// A wave of stream_vad_decide_kernel reads and writes c0 with lane = coefficient: 256 contiguous bytes; the header is read through a
// wave-uniform address and written by lane 0.  A quad of stream_vad_lanes_kernel keeps coefficients 4 pq .. 4 pq + 3 in lane pq: two
// 16-byte accesses per lane, 128 contiguous bytes per stream; the header is read by all four lanes (one address per quad) and written
// by lane pq == 0.  Doubles and bit patterns travel as they stand: a store and load is exact, so a file's decisions do not depend on
// how it was cut into pushes.  vst_unpack / vst_pack alone know the header's slots; the kernels move its ten doubles.
// House rules of the stream kernels: nothing is read back, no atomics (a stream id appears once in a push), plain vector stores.
//
// gfx950, hipcc -O3, for THR 0 .. 3 (in brackets: with the step restated here, before it was shared with vad_lanes_kernel):
// stream_vad_lanes_kernel<14, THR> 72 / 74 / 74 / 80 VGPRs (70 / 74 / 72 / 74), 40 / 40 / 44 / 52 SGPRs (40 / 42 / 44 / 52), 340 / 373 / 385 /
// 422 instructions (358 / 376 / 390 / 442); stream_vad_decide_kernel 78 VGPRs (75), 99 SGPRs, 875 instructions (730: the replay loop now comes
// in two versions, with and without the energy criterion), 16 KB of LDS; stream_vad_rows_kernel 20 VGPRs, 33 SGPRs; stream_vad_finish_kernel
// 24 VGPRs, 43 SGPRs, 161 instructions (the same); no spills, no scratch.  Times against the restated step: profiles/vad_step_ab.txt.
// stream_vad_delayed_kernel 79 VGPRs, 106 SGPRs, 978 instructions, 16 KB of LDS (stream_vad_decide_kernel beside it: 78 / 99 / 875, the
// code it had before the twin existed); stream_vad_delayed_finish_kernel 59 VGPRs, 76 SGPRs, 766 instructions, no LDS; no spills, no
// scratch.  Like stream_vad_decide_kernel the two are coverage, not tuned paths, and no time is claimed for them.
#pragma once

namespace {

constexpr int VST_DOUBLES = 48, VST_C0 = 16;

struct StreamVadParams {
    const RowPush *push;
    const int *replay;     // positions in `push` of the streams that complete a frame (stream_vad_lanes_kernel)
    int n_replay;
    const float *cf;       // fused criterion: cepstra [frames of the push][VFC_STRIDE] (vad_a2c_kernel's output)
    const double *ci;      // Burg criterion: cepstra [frames of the push][ncoef] (vad_burg_kernel's output)
    const float *energy;   // energy criterion: [frames of the push]
    double *vstate;        // [n_streams][VST_DOUBLES]
    uint8_t *vad;          // decision bytes of the push
};

// The scalar header of a record, slots [0 .. VST_HEADER) as the table above has them, to and from registers: the kernels move `hd`
// between registers and memory with the access width of their lanes.
constexpr int VST_HEADER = 10;
__device__ __forceinline__ void vst_unpack(VadThr &s, VadFilter &f, const double (&hd)[VST_HEADER]) {
    s.crimin = hd[0]; s.crimax = hd[1]; s.crimean = hd[2]; s.crimean2 = hd[3]; s.crivar = hd[4]; s.dmin = hd[5]; s.dmax = hd[6];
    f.hist = (unsigned long long)__double_as_longlong(hd[7]);
    s.adapt_vad = __double2loint(hd[8]); f.hidx = __double2hiint(hd[8]);
    f.nsum = __double2loint(hd[9]);
}
__device__ __forceinline__ void vst_pack(const VadThr &s, const VadFilter &f, double (&hd)[VST_HEADER]) {
    hd[0] = s.crimin; hd[1] = s.crimax; hd[2] = s.crimean; hd[3] = s.crimean2; hd[4] = s.crivar; hd[5] = s.dmin; hd[6] = s.dmax;
    hd[7] = __longlong_as_double((long long)f.hist);
    hd[8] = __hiloint2double(f.hidx, s.adapt_vad);
    hd[9] = __hiloint2double(0, f.nsum);
}

// grid ceil(n_replay / 16), 64 lanes: quad q of wave w is the stream at position replay[16 w + q] of the push
template <int NCL, int THR>
__global__ __launch_bounds__(64) void stream_vad_lanes_kernel(const StreamVadParams p, const VadParams vp) {
    const int lane = threadIdx.x, pq = lane & 3;
    const int gidx = blockIdx.x * 16 + (lane >> 2);
    const bool live = gidx < p.n_replay;
    RowPush d;
    d.F0 = d.r0 = d.out0 = d.row0 = 0;
    d.id = d.Tn = d.nr = d.hsel = 0;
    if (live) d = p.push[p.replay[gidx]];
    const int T = live ? d.Tn : 0;  // (> 0 for every listed stream: the host lists those that complete a frame)
    int Tmax = T;
#pragma unroll
    for (int off = 32; off >= 4; off >>= 1) Tmax = max(Tmax, __shfl_xor(Tmax, off, 64));
    const int order_f = vp.filter_order, h = (order_f - 1) / 2;
    VadQuad r = {};
    double *vs = p.vstate + (size_t)d.id * VST_DOUBLES;
    double2 *h2 = reinterpret_cast<double2 *>(vs), *c2 = reinterpret_cast<double2 *>(vs + VST_C0 + 4 * pq);
    if (live && d.F0 > 0) {  // the file goes on: where the stream's last push left off
        double hd[VST_HEADER];
#pragma unroll
        for (int k = 0; k < VST_HEADER / 2; k++) {
            const double2 v = h2[k];
            hd[2 * k] = v.x; hd[2 * k + 1] = v.y;
        }
        vst_unpack(r.thr, r.f, hd);
        const double2 u = c2[0], v = c2[1];
        r.c0[0] = u.x; r.c0[1] = u.y; r.c0[2] = v.x; r.c0[3] = v.y;
    }
    // byte of row k of the file goes to vad[out0 + k - r0]; frame t >= h emits row t - h
    uint8_t *out = p.vad + d.out0 - d.r0;
    const float4 *cf4 = reinterpret_cast<const float4 *>(p.cf + d.row0 * VFC_STRIDE) + pq;
    float4 q = live ? cf4[0] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < Tmax; i++) {
        const double ci[4] = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
        if (i + 1 < T) q = cf4[(size_t)(i + 1) * (VFC_STRIDE / 4)];  // the next frame's cepstra are in flight while this one is worked on
        if (i < T) {  // (a quad is one stream: its four lanes take the branch together, the quad_perm adds stay inside it)
            const long long t = d.F0 + i;
            // the recurrences name frames up to the init counts (ints): beyond 2^30 frames of one file every such branch is long decided
            const int tt = (int)min(t, (long long)0x40000000);
            const int vad0 = vad_quad_step<NCL, THR>(r, vp, tt, ci, pq);
            vad_push(r.f, vad0, order_f);
            if (t >= h && pq == 0) out[t - h] = vad_byte(r.f, order_f);
        }
    }
    if (live) {  // behind the push's last frame
        if (pq == 0) {
            double hd[VST_HEADER];
            vst_pack(r.thr, r.f, hd);
#pragma unroll
            for (int k = 0; k < VST_HEADER / 2; k++) h2[k] = make_double2(hd[2 * k], hd[2 * k + 1]);
        }
        c2[0] = make_double2(r.c0[0], r.c0[1]);
        c2[1] = make_double2(r.c0[2], r.c0[3]);
    }
}

__device__ __forceinline__ void vst_load(VadRun &r, const double *vs, int lane) {
    double hd[VST_HEADER];
#pragma unroll
    for (int k = 0; k < VST_HEADER; k++) hd[k] = vs[k];
    vst_unpack(r.thr, r.f, hd);
    r.c0r = lane < 32 ? vs[VST_C0 + lane] : 0.0;
}
__device__ __forceinline__ void vst_store(const VadRun &r, double *vs, int lane) {
    if (lane == 0) {
        double hd[VST_HEADER];
        vst_pack(r.thr, r.f, hd);
#pragma unroll
        for (int k = 0; k < VST_HEADER; k++) vs[k] = hd[k];
    }
    if (lane < 32) vs[VST_C0 + lane] = r.c0r;
}

// Detector state behind row state (CTU_STREAMS_VAD_ROW_STATE): what the delayed replay reads beside StreamVadParams
struct StreamVadDelay {
    const VadCalls *calls;  // by position in the push: the calls every pushed stream makes now (stream_plan.h)
    double *crec;           // [n_streams][stride]: the criterion input of every stream's newest frame - the energy (as a double: exact), or
                            // the frame's ncoef Burg cepstra.  Stored and reloaded as they stand
    int stride, delay;      // doubles of a record; the chain's halo H
};

// grid (pushed streams), 64 lanes: vad_decide_kernel's replay of the energy (vp.cri 0) and Burg (vp.cri 1) criteria over the frames of
// the push - 64 of them staged in LDS with coalesced loads, then vad_frame one at a time
__global__ __launch_bounds__(64) void stream_vad_decide_kernel(const StreamVadParams p, const VadParams vp) {
    __shared__ double stage[64 * 32];
    const RowPush d = p.push[blockIdx.x];
    const int lane = threadIdx.x;
    const int T = d.Tn;
    if (T == 0) return;  // completes no frame: not touched
    const int nc = vp.cri == 0 ? 1 : vp.ncoef;
    double *vs = p.vstate + (size_t)d.id * VST_DOUBLES;
    VadRun run = {};
    if (d.F0 > 0) vst_load(run, vs, lane);
    // vad_emit writes out[run.nout] and counts on: row k of the file has byte out0 + k - r0 of the push, and R(F0) rows are out
    run.nout = (int)min(d.r0, (long long)0x40000000);
    uint8_t *out = p.vad + d.out0 - run.nout;
    for (int tb = 0; tb < T; tb += 64) {
        const int nt = min(64, T - tb);
        __syncthreads();
        if (vp.cri == 0) {
            if (lane < nt) stage[lane] = p.energy[d.row0 + tb + lane];
        } else {
            for (int e = lane; e < nt * nc; e += 64) stage[e] = p.ci[(d.row0 + tb) * nc + e];
        }
        __syncthreads();
        for (int tt = 0; tt < nt; tt++) {
            const double en = vp.cri == 0 ? stage[tt] : 0.0;
            const double cil = (vp.cri != 0 && lane < nc) ? stage[tt * nc + lane] : 0.0;
            const int t = (int)min(d.F0 + tb + tt, (long long)0x40000000);  // (as in stream_vad_lanes_kernel: the branches that name frames)
            vad_frame(run, vp, t, en, cil, lane, out);
        }
    }
    vst_store(run, vs, lane);
}

// Its delayed twin, behind a delta chain, a stacking or CMS (the same grid): instead of a call per frame the calls c0 .. c0 + nc - 1 of
// q.calls, call j on the criterion of frame j + q.delay - a frame of this push, or (one push of a file at most) the frame ahead of it,
// which is the stream's record - with j the index every branch of the recurrences takes.  A file's first call (c0 == 0) starts from the
// zero state, whichever push makes it; behind the calls the push's newest frame becomes the record.
__global__ __launch_bounds__(64) void stream_vad_delayed_kernel(const StreamVadParams p, const VadParams vp, const StreamVadDelay q) {
    __shared__ double stage[64 * 32];
    const RowPush d = p.push[blockIdx.x];
    const int lane = threadIdx.x;
    const int T = d.Tn;
    if (T == 0) return;  // completes no frame: neither a call nor a newer record
    const int nc = vp.cri == 0 ? 1 : vp.ncoef;
    double *vs = p.vstate + (size_t)d.id * VST_DOUBLES, *rec = q.crec + (size_t)d.id * q.stride;
    const VadCalls c = q.calls[blockIdx.x];
    const int first = (int)(c.c0 + q.delay - d.F0);  // the push's frame call c0 reads (-1: the one ahead of it); the last call reads frame T - 1
    VadRun run = {};
    if (c.c0 > 0) vst_load(run, vs, lane);
    run.nout = (int)min(d.r0, (long long)0x40000000);  // (as above; R(F0) = max(c0 - h, 0) is the host's)
    uint8_t *out = p.vad + d.out0 - run.nout;
    for (int tb = 0; tb < c.nc; tb += 64) {
        const int nt = min(64, c.nc - tb);
        __syncthreads();
        if (vp.cri == 0) {
            if (lane < nt) {
                const int f = first + tb + lane;
                stage[lane] = f < 0 ? rec[0] : (double)p.energy[d.row0 + f];
            }
        } else {
            for (int e = lane; e < nt * nc; e += 64) {
                const int k = e / nc, i = e - k * nc, f = first + tb + k;
                stage[e] = f < 0 ? rec[i] : p.ci[(d.row0 + f) * nc + i];
            }
        }
        __syncthreads();
        for (int tt = 0; tt < nt; tt++) {
            const double en = vp.cri == 0 ? stage[tt] : 0.0;
            const double cil = (vp.cri != 0 && lane < nc) ? stage[tt * nc + lane] : 0.0;
            const int t = (int)min(c.c0 + tb + tt, (long long)0x40000000);
            vad_frame(run, vp, t, en, cil, lane, out);
        }
    }
    if (c.nc > 0) vst_store(run, vs, lane);
    // frame F0 + T - 1 is the file's newest (the record was read ahead of the first barrier above, by this wave)
    if (vp.cri == 0) {
        if (lane == 0) rec[0] = (double)p.energy[d.row0 + T - 1];
    } else if (lane < nc) rec[lane] = p.ci[(d.row0 + T - 1) * nc + lane];
}

// grid (64-row chunks of the stream with the most rows, pushed streams), 256 lanes
__global__ __launch_bounds__(256) void stream_vad_rows_kernel(const RowParams p, const int D) {
    const RowPush d = p.push[blockIdx.y];
    const long long i0 = 64LL * blockIdx.x;
    if (i0 >= d.nr) return;
    const int nout = (int)min(64LL, d.nr - i0);
    float *out = p.rows + (d.out0 + i0) * D;
    for (int e = threadIdx.x; e < nout * D; e += 256) {
        const int r = e / D, c = e - r * D;
        out[e] = stream_base_row(p, d, d.r0 + i0 + r)[c];
    }
}

// One workgroup, 256 lanes: the stream that finishes (p.push[0]: F0 = the file's frames, Tn = 0, r0 = R(F0), nr = min(F0, h) > 0).
// The held rows come from the history alone; lane 0 pushes vad_flush's zeros through the filter (src/vad/vad.h:156-175) for their bytes.
// The stream's record is left as it stands: the next file's first push starts from the zero state.
__global__ __launch_bounds__(256) void stream_vad_finish_kernel(const RowParams p, const int D, const double *__restrict__ vstate, uint8_t *__restrict__ vad,
                                                                 const int order) {
    const RowPush d = p.push[0];
    if (p.rows)
        for (int e = threadIdx.x; e < d.nr * D; e += 256) {
            const int r = e / D, c = e - r * D;
            p.rows[(d.out0 + r) * D + c] = stream_base_row(p, d, d.r0 + r)[c];
        }
    if (threadIdx.x == 0 && vad) {
        const double *vs = vstate + (size_t)d.id * VST_DOUBLES;
        double hd[VST_HEADER];
#pragma unroll
        for (int k = 0; k < VST_HEADER; k++) hd[k] = vs[k];
        VadThr thr;  // (not used: the filter's three fields are all that is read)
        VadFilter f;
        vst_unpack(thr, f, hd);
        for (int k = 0; k < d.nr; k++) {  // vad_flush: k < h && nout < T
            vad_push(f, 0, order);
            vad[d.out0 + k] = vad_byte(f, order);
        }
    }
}

// Its twin behind row state.  One wave: the stream that finishes (p.push[0]: F0 = the file's frames T, Tn = 0, r0 = R(T), nr = T - r0 > 0,
// so T > h) makes the calls the file still owes, c.c0 = C(T) .. T - 1 - all of them where T <= delay - each on the criterion of frame
// T - 1, which is the stream's record (vad_decide_kernel's min(j + delay, T - 1)); then vad_flush's zeros.  Bytes r0 .. T - 1 of the file
// are bytes 0 .. nr - 1 of the call.  The rows are the row kernels' (finishing); record and state are left as they stand.
__global__ __launch_bounds__(64) void stream_vad_delayed_finish_kernel(const StreamVadParams p, const VadParams vp, const StreamVadDelay q, const VadCalls c) {
    const RowPush d = p.push[0];
    const int lane = threadIdx.x;
    const int nc = vp.cri == 0 ? 1 : vp.ncoef;
    VadRun run = {};
    if (c.c0 > 0) vst_load(run, p.vstate + (size_t)d.id * VST_DOUBLES, lane);
    run.nout = (int)min(d.r0, (long long)0x40000000);
    uint8_t *out = p.vad + d.out0 - run.nout;
    const int end = run.nout + d.nr;  // (the file's length, but for the clamp of nout)
    const double *rec = q.crec + (size_t)d.id * q.stride;
    const double en = vp.cri == 0 ? rec[0] : 0.0;
    const double cil = (vp.cri != 0 && lane < nc) ? rec[lane] : 0.0;
    for (int k = 0; k < c.nc; k++) {
        const int t = (int)min(c.c0 + k, (long long)0x40000000);
        vad_frame(run, vp, t, en, cil, lane, out);
    }
    vad_flush(run, vp, end, lane, out);
}

}  // namespace
