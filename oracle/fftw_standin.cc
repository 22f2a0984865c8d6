// The three r2r transforms of oracle/fftw_standin/fftw3.h as direct sums in long double, rounded once to double.
//   R2HC     X_k = sum_j x_j exp(-2 pi i j k / n), out[k] = Re X_k (k = 0 .. n/2), out[n-k] = Im X_k (0 < k < n/2); unnormalised
//   HC2R     its unnormalised inverse: x_j = X_0 + (-1)^j X_{n/2} [n even] + 2 sum_{0<k<n/2} (Re X_k cos(2 pi j k / n) - Im X_k sin(2 pi j k / n))
//   REDFT10  Y_k = 2 sum_j x_j cos(pi (j + 1/2) k / n)
// Every angle is a multiple of 2 pi / period (period = n, or 4 n for REDFT10), so one table of `period` long-double cosines and sines,
// indexed by the multiple reduced modulo the period, serves a plan: no argument grows with j k.
#include "fftw_standin/fftw3.h"

#include <cmath>
#include <cstdlib>
#include <vector>

struct ctu_standin_plan {
    int n;
    double *in, *out;
    fftw_r2r_kind kind;
    std::vector<long double> c, s;   // cos / sin (2 pi m / period)
    std::vector<long double> acc;    // results of one execution: in may be out
};

extern "C" {

void *fftw_malloc(size_t n) { return std::malloc(n ? n : 1); }

void fftw_free(void *p) { std::free(p); }

fftw_plan fftw_plan_r2r_1d(int n, double *in, double *out, fftw_r2r_kind kind, unsigned) {
    if (n < 1 || (kind != FFTW_R2HC && kind != FFTW_HC2R && kind != FFTW_REDFT10)) return nullptr;
    ctu_standin_plan *p = new ctu_standin_plan;
    p->n = n;
    p->in = in;
    p->out = out;
    p->kind = kind;
    const long period = kind == FFTW_REDFT10 ? 4L * n : n;
    const long double two_pi = 8.0L * atanl(1.0L);
    p->c.resize(period);
    p->s.resize(period);
    for (long m = 0; m < period; m++) {
        p->c[m] = cosl(two_pi * (long double)m / (long double)period);
        p->s[m] = sinl(two_pi * (long double)m / (long double)period);
    }
    p->acc.resize(n);
    return p;
}

void fftw_execute(const fftw_plan p) {
    const long n = p->n;
    const double *x = p->in;
    std::vector<long double> &y = p->acc;
    if (p->kind == FFTW_R2HC) {
        for (long k = 0; k <= n / 2; k++) {
            long double re = 0.0L, im = 0.0L;
            long m = 0;                                  // j k mod n
            for (long j = 0; j < n; j++) {
                re += (long double)x[j] * p->c[m];
                im -= (long double)x[j] * p->s[m];
                m += k;
                if (m >= n) m -= n;
            }
            y[k] = re;
            if (k > 0 && 2 * k < n) y[n - k] = im;
        }
    } else if (p->kind == FFTW_HC2R) {
        for (long j = 0; j < n; j++) {
            long double a = (long double)x[0];
            if (n % 2 == 0 && n > 1) a += (j % 2 ? -1.0L : 1.0L) * (long double)x[n / 2];
            long double b = 0.0L;
            long m = 0;                                  // j k mod n
            for (long k = 1; 2 * k < n; k++) {
                m += j;
                if (m >= n) m -= n;
                b += (long double)x[k] * p->c[m] - (long double)x[n - k] * p->s[m];
            }
            y[j] = a + 2.0L * b;
        }
    } else {
        const long period = 4 * n;
        for (long k = 0; k < n; k++) {
            long double a = 0.0L;
            long m = k % period;                         // (2 j + 1) k mod 4 n
            const long step = (2 * k) % period;
            for (long j = 0; j < n; j++) {
                a += (long double)x[j] * p->c[m];
                m += step;
                if (m >= period) m -= period;
            }
            y[k] = 2.0L * a;
        }
    }
    for (long i = 0; i < n; i++) p->out[i] = (double)y[i];
}

void fftw_destroy_plan(fftw_plan p) { delete p; }

}  // extern "C"
