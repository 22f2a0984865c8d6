// Streaming input with trap state (include/ctu_engine.h: CTU_STREAMS_TRAP_STATE): TRAP-DCT behind the front end of a push.
// Included by engine.hip behind trap_kernel.h, whose contraction this kernel evaluates by absolute frame index, and behind
// stream_rows_kernels.h, whose descriptors, histories and carry it shares.
//
// out[t][b*ndct+k] = sum_j G[k][j] * logmel[clamp(t-half+j, 0, T-1)][b], half = (traplen-1)/2: row t is final once frame t + half
// exists, so after F frames of a file rows 0 .. F-half-1 have gone out (none while F <= half: stream_trap_halo) and the last half
// rows wait for ctu_streams_finish, which runs the same kernel with the file's length known.  Log-mel rows come from two places, as the
// base rows of stream_rows_kernels.h do: the frames of this push from the dense rows the front end has just written (the plan's logmel,
// band_to_scratch = 1 as offline), the frames before it from the stream's history - the last C = 2 half log-mel rows of the file, [B]
// floats each, which stream_rows_carry_kernel moves on (Dbase = B).  A push delivers from row F0 - half on, which reads from F0 - 2 half on.
//
//   stream_trap_kernel<NRB>   the rows that go out with a push, or with a finish: trapdct_mfma_kernel's exact-fp32 contraction
//                             D[k][col] += G[k][4s..4s+3] * X[4s..4s+3][col] on v_mfma_f32_16x16x4_f32, tap j = 4s + (lane>>4), s ascending
//                             from a zero accumulator, operand x[f][b] - x[t][b] (the column's own centre value).  NRB row blocks of 16
//                             DCT coefficients (ndct <= 16 NRB), as offline.  COMP, for contexts of more than 104 frames, below.
//
// Mapping.  A push brings many streams and a handful of frames each, so the 16 columns of an MFMA are 16 output rows of the push in
// the order of the caller's buffer - (stream, row) pairs, whatever streams they belong to - not 16 consecutive frames of one file: a
// push of one frame to 1024 streams fills its columns as an offline run does.  The host tabulates the stream of every column
// (stream_trap_columns, stream_plan.h); column c is row c of the caller's buffer.  A workgroup is one wave: 16 columns and a block of
// BB bands (grid.y walks the band blocks: 8 bands with one row block, 4 with two), so a small push still spreads over the chip.
// A column's result depends on nothing but its own traplen log-mel rows: not on which column of which wave computes it, not on how
// the file was cut into pushes, not on the other streams - and it is the offline fp32 kernel's bit for bit when the log-mel rows are.
//
// The B operand comes straight from the L2-resident rows, no LDS: per tap group a lane computes its row's address once (clamp, fresh or
// history, 64-bit offset) and loads BB consecutive floats of it, one tap group ahead of the MFMAs that use them; the accumulators are
// 4 BB NRB = 32 registers, the operands of two tap groups and the centre values 3 BB.  G is read as it is needed (one guarded load per
// row block and tap group, L1 / L2 hits: ndct * traplen floats at most 32 KB for the whole grid).
//
// Long contexts (COMP: more than TRAP_COMP_STEPS = 26 tap groups, traplen 105 .. 255).  Up to 26 tap groups the arithmetic is the
// offline kernel's short instantiation and the rows are its rows bit for bit.  Beyond, one fp32 accumulator chain over the whole context
// does not hold the engine's parity bound (1.9e-4 of max(|oracle|, 1) on 140 frames of speech at 255 taps, against 1e-4), so there the
// accumulator is closed every TRAP_COMP_RUN = 2 tap groups (8 taps) into a sum kept as two floats: trap_comp_close and trap_comp_row
// of trap_kernel.h, which say how and why - and which the offline kernel's long instantiations (trapdct_mfma_kernel<NRB, 64>) call as
// well, on the same ascending taps and the same centred operand, so the identity with the offline rows holds at these sizes too.  A
// column still depends on its own traplen log-mel rows alone - not on the cut into pushes, not on the other streams.  64 more registers
// (hi, lo) and 12 VALU operations per accumulator register and run.
//
// What is guarded: a tap beyond traplen (4 ceil(traplen/4) > traplen, traplen is odd) has a zero in G, as offline (areg), and a zero
// for its operand too - the frame it would name is no part of the row's context, and on an all-zero frame (digital silence: the
// logarithm of an empty band, -inf) 0 x -inf would make the row NaN where the reference's is finite.  Its fetch still needs an address
// that exists, and mid-stream the row it would name lies beyond the newest frame: the fetch index is clamped to
// [first frame in reach, newest frame], both of which exist.  That upper clamp is the right-hand clamp T-1 of a finish (the newest frame
// is the file's last); mid-stream no real tap of a row that goes out reaches it.  The left clamp at frame 0 is applied to the index ahead
// of the address: frames below 0 are in no history.  Idle columns (beyond the push's rows) neither load nor store.
// Every count is the host's (RowPush): nothing is read back between pushes.  Plain vector loads and stores, no atomics: a stream id
// appears once in a push.
//
// gfx950, hipcc -O3: stream_trap_kernel<1, false> 76 VGPRs, 32 AGPRs (the accumulators), 54 SGPRs; <2, false> 66 VGPRs, 32 AGPRs,
// 48 SGPRs; four waves per SIMD each.  <1, true> 144 VGPRs, 32 AGPRs, 70 SGPRs (two waves per SIMD); <2, true> 124 VGPRs, 32 AGPRs,
// 54 SGPRs (three).  No spills, no scratch, no LDS in any of them.
#pragma once

namespace {

// (TRAP_COMP_STEPS, TRAP_COMP_RUN: layout_constants.h)

struct StreamTrapParams {
    const RowPush *push;
    const int *col;      // the position in the push of every column's stream (stream_trap_columns)
    const float *fresh;  // the push's new log-mel rows [frames][B]
    const float *hist;   // [2][n_streams][C][B]
    const float *G;      // [ndct][traplen]
    float *rows;         // the caller's
    long long n_cols;    // rows that go out
    int n_streams, C, B, traplen, ndct, D;
};

// grid (16-column groups of the rows that go out, blocks of BB bands), 64 lanes
template <int NRB, bool COMP>  // COMP: contexts beyond the offline kernel's short instantiation (more than TRAP_COMP_STEPS tap groups)
__global__ __launch_bounds__(64) void stream_trap_kernel(const StreamTrapParams p) {
    constexpr int BB = NRB == 1 ? 8 : 4;
    const int lane = threadIdx.x, cn = lane & 15, q = lane >> 4;
    const long long c = 16LL * blockIdx.x + cn;
    const bool live = c < p.n_cols;
    const int b0 = blockIdx.y * BB, nb = min(BB, p.B - b0);
    const int half = (p.traplen - 1) / 2, nsteps = (p.traplen + 3) / 4;
    // This lane's column: frames count from F0, the first one of this push (rel < 0: the history's).  lo .. hi are the frames that
    // exist and are in reach: frame 0 or the history's oldest, and the newest one (Tn = 0 when finishing: the file's last, F0 - 1).
    int trel = 0, lo = 0, hi = 0;
    long long frow = 0, hrow = 0;
    if (live) {
        const RowPush d = p.push[p.col[c]];
        trel = (int)(d.r0 + (c - d.out0) - d.F0);
        lo = -(int)min(d.F0, (long long)p.C);
        hi = d.Tn - 1;
        frow = d.row0;
        hrow = ((long long)d.hsel * p.n_streams + d.id) * p.C + p.C;
    }
    auto row_of = [&](int rel) -> const float * {  // stream_base_row's addressing, behind the clamps
        rel = min(max(rel, lo), hi);
        return (rel >= 0 ? p.fresh : p.hist) + ((rel >= 0 ? frow : hrow) + rel) * (long long)p.B + b0;
    };
    auto fetch = [&](int rel, float (&x)[BB]) {
        const float *r = row_of(rel);
#pragma unroll
        for (int bb = 0; bb < BB; bb++) x[bb] = (live && bb < nb) ? r[bb] : 0.f;
    };
    float xc[BB], xn[BB];
    fetch(trel, xc);
    fetch(trel - half + q, xn);
    f32x4 acc[BB][NRB];
#pragma unroll
    for (int bb = 0; bb < BB; bb++)
#pragma unroll
        for (int rb = 0; rb < NRB; rb++) acc[bb][rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 sum_hi[BB][NRB], sum_lo[BB][NRB];  // (COMP) the closed runs of tap groups as an unevaluated sum of two floats
    if constexpr (COMP) {
#pragma unroll
        for (int bb = 0; bb < BB; bb++)
#pragma unroll
            for (int rb = 0; rb < NRB; rb++) sum_hi[bb][rb] = sum_lo[bb][rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int s_ = 0; s_ < nsteps; s_++) {
        float x[BB], a[NRB];
        const int j = 4 * s_ + q;
        // a tap beyond traplen is no tap: its operand is zero like its weight, whatever the frame it would name holds (0 x -inf is NaN)
#pragma unroll
        for (int bb = 0; bb < BB; bb++) x[bb] = j < p.traplen ? xn[bb] - xc[bb] : 0.f;
        // this lane's slice of G: A[i = lane&15][k = lane>>4] of the 16x4 block, zero beyond ndct and traplen (trapdct_mfma_kernel's areg)
#pragma unroll
        for (int rb = 0; rb < NRB; rb++) {
            const int k = rb * 16 + cn;
            a[rb] = (k < p.ndct && j < p.traplen) ? p.G[k * p.traplen + j] : 0.f;
        }
        if (s_ + 1 < nsteps) fetch(trel - half + j + 4, xn);  // the next tap group's rows, ahead of this one's MFMAs
#pragma unroll
        for (int bb = 0; bb < BB; bb++)
            if (bb < nb) {
#pragma unroll
                for (int rb = 0; rb < NRB; rb++) acc[bb][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], x[bb], acc[bb][rb], 0, 0, 0);
            }
        if constexpr (COMP) {
            // every TRAP_COMP_RUN tap groups, and behind the last: the accumulator joins the sum by an error-free addition and starts
            // over from zero, so no chain is longer than a run (trap_comp_close, trap_kernel.h: the offline kernel's long contexts too)
            if (trap_comp_closes(s_, nsteps)) {
#pragma unroll
                for (int bb = 0; bb < BB; bb++)
                    if (bb < nb) {
#pragma unroll
                        for (int rb = 0; rb < NRB; rb++) trap_comp_close(acc[bb][rb], sum_hi[bb][rb], sum_lo[bb][rb]);
                    }
            }
        }
    }
    if constexpr (COMP) {
#pragma unroll
        for (int bb = 0; bb < BB; bb++)
#pragma unroll
            for (int rb = 0; rb < NRB; rb++) acc[bb][rb] = trap_comp_row(sum_hi[bb][rb], sum_lo[bb][rb]);
    }
    if (!live) return;
    float *out = p.rows + c * p.D;  // column c is row c of the caller's buffer (out0 is the prefix sum of nr)
#pragma unroll
    for (int bb = 0; bb < BB; bb++) {
        if (bb >= nb) break;
        const int b = b0 + bb;
        if (NRB == 1 && p.ndct == 16 && (p.D & 3) == 0) {
            // C/D layout: this lane holds coefficients 4*(lane>>4)..+3 of column lane&15: one 16-byte store
            *reinterpret_cast<f32x4 *>(out + b * 16 + q * 4) = acc[bb][0];
        } else {
            float *o = out + b * p.ndct;
#pragma unroll
            for (int rb = 0; rb < NRB; rb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int k = rb * 16 + q * 4 + r;  // C/D layout: row = (lane>>4)*4 + reg, col = lane&15
                    if (k < p.ndct) o[k] = acc[bb][rb][r];
                }
        }
    }
}

}  // namespace
