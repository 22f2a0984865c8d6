// Streaming input with row state (include/ctu_engine.h: CTU_STREAMS_ROW_STATE): the delta chain / stacking and CMS behind the front end
// of a push.  Included by engine.hip behind post_kernels.h, whose formulas these kernels evaluate by absolute frame index.
//
// post_kernel and the cms kernels know a file's length T when they run.  A push does not, and does not need to: every place where T
// enters their formulas - the right-hand clamp min(f, T-1), the zero a stage of window 1 emits for frame T-1, the stacking rows
// T-w .. T-1 and E of frame min(t+H, T-1) - is reached only by rows t >= T - H (H: the sum of the chain's windows, or the stacking
// window).  So after F frames of a file, rows 0 .. F-H-1 are final whatever follows, and they go out; the others wait for the push
// that brings H more frames or for ctu_streams_finish, which runs the same kernels with T = F.  No row goes out before frame wmax+2
// exists (wmax: the largest window): a file that ends sooner has no defined rows (the plan's refusal), and finish says so.
//
// Base rows come from two places: the frames of this push from the dense rows the front end and its tails have just written
// (lp_tail_kernel and dct_wide_kernel walk rows 0 .. total_frames of a run by index, so those stay one dense run), the frames before
// it from the stream's history - the last C = max(2H, H+L-1) base rows of the file (L: the block-CMS window, else 1): a push delivers
// from row F0-H on, which reads base rows from F0-2H on, and block CMS of that row reads base rows from F0-H-L+1 on.
//
//   stream_post_kernel        rows r0 .. r0+nr-1 of every pushed stream: post_kernel's delta stages (ascending i, difference first,
//                             then inv_den) or its stacking, left clamp at frame 0, right clamp only when finishing
//   stream_cms_exp_kernel     cms_exp_kernel's __fmul_rn / __fmaf_rn pair along those rows, the mean per column and stream carried in HBM
//   stream_cms_block_kernel   cms_block_kernel's ring-order sum over base rows t-L+1 .. t
//   stream_rows_carry_kernel  the last C base rows into the stream's other history (two per stream, taken in turn: a shift in place
//                             would read what another lane overwrites)
// Every count a kernel uses is the host's (RowPush): nothing is read back between pushes.  Plain loads and stores, no atomics: a stream id
// appears once in a push.
//
// gfx950, hipcc -O3: stream_post_kernel 46 VGPRs, 60 SGPRs (delta chain) / 56 SGPRs (stacking); stream_cms_exp_kernel 9 VGPRs, 61 SGPRs;
// stream_cms_block_kernel 58 VGPRs, 65 SGPRs; stream_rows_carry_kernel 12 VGPRs, 25 SGPRs; no spills, no scratch.  LDS is dynamic and
// the size post_kernel / cms_block_kernel take: (64 + 2H) (Dbase + order fea_c) floats, (64 + L - 1) ncols floats; none in the other two.
#pragma once

#include "stream_plan.h"  // RowPush: the host plans a push by it

namespace {

constexpr int STREAM_MEANS = 32;  // CMS columns at most (accept.cc: "more than 32 CMS columns")

struct RowParams {
    const RowPush *push;
    const float *fresh;  // the push's new base rows [frames][Dbase]
    float *hist;         // [2][n_streams][C][Dbase]
    float *means;        // [n_streams][STREAM_MEANS]
    float *rows;         // the caller's
    int n_streams, C, Dbase;
    int finishing;       // the file's length is F0 + Tn
};

// base row f of the file, F0 - C <= f < F0 + Tn
__device__ __forceinline__ const float *stream_base_row(const RowParams &p, const RowPush &d, const long long f) {
    if (f >= d.F0) return p.fresh + (d.row0 + (f - d.F0)) * p.Dbase;
    return p.hist + (((size_t)d.hsel * p.n_streams + d.id) * p.C + (size_t)(f - d.F0 + p.C)) * p.Dbase;
}

// grid (64-row chunks of the stream with the most rows, pushed streams), 256 lanes
template <bool STACK>  // -fea_trap, else the delta chain: two kernels, each with the scalar registers of its own branch
__global__ __launch_bounds__(256) void stream_post_kernel(const RowParams p, const PostParams pp) {
    extern __shared__ float spm[];
    const RowPush d = p.push[blockIdx.y];
    const int fc = pp.fea_c, Db = pp.Dbase, D = pp.D, order_ = pp.order;
    const int H = STACK ? pp.w[0] : pp.w[0] + (order_ > 1 ? pp.w[1] : 0) + (order_ > 2 ? pp.w[2] : 0);
    const int R = 64 + 2 * H;
    float *x0 = spm;                   // [R][Db]   base rows (E column included)
    float *lv = spm + (size_t)R * Db;  // levels 1..order: [R][fc] each
    const long long F1 = d.F0 + d.Tn, rend = d.r0 + d.nr;
    const long long t0 = d.r0 + 64LL * blockIdx.x;
    if (t0 >= rend) return;
    {
        const int nout = (int)min(64LL, rend - t0);
        // Frames of this chunk count from tlo, the first one its LDS image has room for: frame f is image row f - tlo, and post_kernel's
        // formulas below are in those terms.  zero / last: frame 0 and the file's last frame T - 1, where they are in reach (mid-stream the
        // file ends beyond every frame a row that goes out reads: F1 - 1 - tlo < 2^30 there, a push has at most 2^26 frames).
        const long long tlo = t0 - H;
        const int newest = (int)(F1 - 1 - tlo);
        const int zero = tlo <= 0 ? (int)-tlo : -1, rmin = max(zero, 0), last = p.finishing ? newest : 0x40000000;
        {
            const int n = (min(nout - 1 + 2 * H, newest) - rmin + 1) * Db;
            for (int e = threadIdx.x; e < n; e += 256) {
                const int r = e / Db, c = e - r * Db;
                x0[(size_t)(rmin + r) * Db + c] = stream_base_row(p, d, tlo + rmin + r)[c];
            }
        }
        __syncthreads();
        auto rowof = [&](int f) { return min(max(f, rmin), last); };
        float *out = p.rows + (d.out0 + (t0 - d.r0)) * D;
        if constexpr (STACK) {
            const int w = pp.w[0], L = 2 * w + 1, xs = fc * L;
            for (int e = threadIdx.x; e < nout * D; e += 256) {
                const int tt = e / D, k = e - tt * D;
                const int t = H + tt;
                float v;
                if (k == xs) v = x0[(size_t)rowof(t + w) * Db + fc];  // E
                else {
                    int i, f;
                    if (k < fc && (t == zero || t > last - w)) { i = k; f = t; }
                    else {
                        i = k / L;
                        const int j = k - i * L;
                        if (t == zero) f = zero + (j < w ? 0 : max(1, j - w));
                        else if (w == 1 && t == last) f = last;
                        else f = t - w + j;
                    }
                    v = x0[(size_t)rowof(f) * Db + (i == 0 ? fc - 1 : i - 1)];
                }
                out[e] = v;
            }
        } else {
            int hk = H;
            const float *prev = x0;
            int pstride = Db;
#pragma unroll 1
            for (int k = 0; k < order_; k++) {
                const int w = pp.w[k];
                hk -= w;  // halo this level still needs for the stages after it
                float *cur = lv + (size_t)k * R * fc;
                const int flo = max(H - hk, rmin), fhi = min(H + nout - 1 + hk, newest);
                const int n = (fhi - flo + 1) * fc;
                for (int e = threadIdx.x; e < n; e += 256) {
                    const int ff = e / fc, cc = e - ff * fc;
                    const int f = flo + ff;
                    float acc = 0.f;
#pragma unroll 1
                    for (int i = 1; i <= w; i++)
                        acc += (float)i * (prev[(size_t)rowof(f + i) * pstride + cc] - prev[(size_t)rowof(f - i) * pstride + cc]);
                    acc *= pp.inv_den[k];
                    if (w == 1 && f == last) acc = 0.f;
                    cur[(size_t)f * fc + cc] = acc;
                }
                __syncthreads();
                prev = cur;
                pstride = fc;
            }
            const int xs = fc * (order_ + 1);
            for (int e = threadIdx.x; e < nout * D; e += 256) {
                const int tt = e / D, k = e - tt * D;
                const int t = H + tt;
                float v;
                if (k == xs) v = x0[(size_t)rowof(t + H) * Db + fc];  // E
                else {
                    const int j = (k >= fc) + (k >= 2 * fc) + (k >= 3 * fc), cc = k - j * fc;
                    v = j == 0 ? x0[(size_t)t * Db + cc] : lv[((size_t)(j - 1) * R + t) * fc + cc];
                }
                out[e] = v;
            }
        }
    }
}

// grid (pushed streams), 64 lanes: lanes 0..31 a CMS column each along the rows, lanes 32..63 the other base columns when no delta
// pass wrote them
__global__ __launch_bounds__(64) void stream_cms_exp_kernel(const RowParams p, const CmsParams cp) {
    const RowPush d = p.push[blockIdx.x];
    if (d.nr == 0) return;
    float *dst = p.rows + d.out0 * cp.D;
    const int c = threadIdx.x;
    if (c < cp.ncols) {
        float *mp = p.means + (size_t)d.id * STREAM_MEANS + c;
        float m = *mp;  // 0 at a file's start (create and finish clear it)
        for (int i = 0; i < d.nr; i++) {
            const float f = stream_base_row(p, d, d.r0 + i)[c];
            m = __fmaf_rn(f, cp.omz, __fmul_rn(m, cp.z));
            dst[(size_t)i * cp.D + c] = f - m;
        }
        *mp = m;
    } else if (c >= 32 && cp.copy_rest) {
        for (int k = cp.ncols + c - 32; k < cp.Dbase; k += 32)
            for (int i = 0; i < d.nr; i++) dst[(size_t)i * cp.D + k] = stream_base_row(p, d, d.r0 + i)[k];
    }
}

// grid (64-row chunks of the stream with the most rows, pushed streams), 256 lanes; LDS [64 + L - 1][ncols]
__global__ __launch_bounds__(256) void stream_cms_block_kernel(const RowParams p, const CmsParams cp) {
    extern __shared__ float scm[];
    const RowPush d = p.push[blockIdx.y];
    const int L = cp.L, nc = cp.ncols;
    const long long rend = d.r0 + d.nr;
    const long long t0 = d.r0 + 64LL * blockIdx.x;
    if (t0 >= rend) return;
    {
        const int nout = (int)min(64LL, rend - t0);
        const long long flo = max(t0 - (L - 1), 0LL);
        const int nrow = (int)(t0 + nout - flo);
        for (int e = threadIdx.x; e < nrow * nc; e += 256) {
            const int r = e / nc, c = e - r * nc;
            scm[e] = stream_base_row(p, d, flo + r)[c];
        }
        __syncthreads();
        float *out = p.rows + (d.out0 + (t0 - d.r0)) * cp.D;
        for (int e = threadIdx.x; e < nout * nc; e += 256) {
            const int tt = e / nc, c = e - tt * nc;
            const long long t = t0 + tt;
            const float f = scm[(int)(t - flo) * nc + c];
            float m = 0.f;
            if (t >= L - 1) {  // cms_block_kernel's order: the frames of the current ring cycle, then the tail of the previous one
                const int tm = (int)(t % L);
                const float *q = scm + (int)(t - tm - flo) * nc + c;
                for (int i = 0; i <= tm; i++) m += q[i * nc];
                q = scm + (int)(t - L + 1 - flo) * nc + c;
                const int n2 = L - 1 - tm;
                for (int i = 0; i < n2; i++) m += q[i * nc];
                m = m / (float)L;
            }
            out[(size_t)tt * cp.D + c] = f - m;
        }
        if (cp.copy_rest)
            for (int e = threadIdx.x; e < nout * (cp.Dbase - nc); e += 256) {
                const int tt = e / (cp.Dbase - nc), c = nc + e - tt * (cp.Dbase - nc);
                out[(size_t)tt * cp.D + c] = stream_base_row(p, d, t0 + tt)[c];
            }
    }
}

// grid (pushed streams, slices of 256 history floats), 256 lanes: frames F1 - C .. F1 - 1 into the other history
__global__ __launch_bounds__(256) void stream_rows_carry_kernel(const RowParams p) {
    const RowPush d = p.push[blockIdx.x];
    if (d.Tn == 0) return;  // the history stands
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= p.C * p.Dbase) return;
    const int j = e / p.Dbase, c = e - j * p.Dbase;
    const long long f = d.F0 + d.Tn - p.C + j;
    if (f < 0) return;  // ahead of the file's start: never read
    p.hist[(((size_t)(d.hsel ^ 1) * p.n_streams + d.id) * p.C + j) * p.Dbase + c] = stream_base_row(p, d, f)[c];
}

}  // namespace
