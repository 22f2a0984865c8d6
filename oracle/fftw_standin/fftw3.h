/* Stand-in for the sliver of the FFTW 3 API that the reference uses, so that a reference tree compiles without the library:
 * fftw_malloc / fftw_free, fftw_plan_r2r_1d for the kinds R2HC, HC2R and REDFT10, fftw_execute, fftw_destroy_plan.
 * Written from the r2r definitions of the FFTW manual ("1d Real-even DFTs", "The Halfcomplex-format DFT"); the transforms
 * are direct O(n^2) sums accumulated in long double (oracle/fftw_standin.cc).  TEST INFRASTRUCTURE ONLY. */
#ifndef CTU_FFTW_STANDIN_H
#define CTU_FFTW_STANDIN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctu_standin_plan *fftw_plan;

/* the numbering of <fftw3.h>; only these three kinds are implemented */
typedef enum { FFTW_R2HC = 0, FFTW_HC2R = 1, FFTW_REDFT10 = 5 } fftw_r2r_kind;

#define FFTW_MEASURE (0U)

void *fftw_malloc(size_t n);
void fftw_free(void *p);
/* NULL for n < 1 or a kind other than the three above.  Planning leaves `in` and `out` untouched, and so does executing HC2R with its input. */
fftw_plan fftw_plan_r2r_1d(int n, double *in, double *out, fftw_r2r_kind kind, unsigned flags);
void fftw_execute(const fftw_plan p);
void fftw_destroy_plan(fftw_plan p);

#ifdef __cplusplus
}
#endif
#endif
