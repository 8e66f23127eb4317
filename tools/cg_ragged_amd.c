/*
 * Conjugate gradient on a symmetric matrix with very unequal row lengths, read from a Matrix Market file, written against the
 * C ABI only: a solver's graph-captured iteration (spgpu/device_scalars.h) on a matrix the library has ADOPTED
 * (spgpuHellSpmvAdopt, spgpu/tuning.h) -- with and without a hold (spgpu/ext/graph.h).
 *
 * The matrix is converted to HELL with the rows as they come (no row order) and adopted.  Then k CG iterations, three ways, all
 * with the scalars on the device (per iteration: spgpuDhellspmv, spgpuDdotDevice, two spgpuDaxpbyQuotDevice, spgpuDdotDevice,
 * spgpuDaxpbyQuotDevice -- the fused spgpuDhellspmvDotDevice has no ordered or adopted form):
 *   1. eager: every call on the handle's stream, the SpMV on the library's ordered copy;
 *   2. one captured graph per parity of |r|^2, no hold: the captured SpMV runs the plain kernel on the caller's arrays
 *      (another order of additions: not necessarily the bits of run 1);
 *   3. the same with a hold on the matrix: the captured SpMV runs on the copy, and the iterate is run 1's bit for bit.
 * Prints the time per iteration of each run, whether runs 2 and 3 repeat run 1 bit for bit (x and |r|^2), and
 * spgpuSpmvAdoptedUses around each capture (run 3's two captures must raise it by exactly 2, run 2's by 0).
 *
 *   usage: cg_ragged_amd matrix.mtx [iterations=50]
 * Exits non-zero (FAILED) if the residual does not fall, run 3 differs from run 1, or the counts are not as above.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/device_scalars.h"
#include "spgpu/ell_conv.h"
#include "spgpu/ext/graph.h"
#include "spgpu/hell.h"
#include "spgpu/hell_conv.h"
#include "spgpu/mmread.h"
#include "spgpu/tuning.h"
#include "spgpu/vector.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

enum { RR_A, RR_B, PAP, SCALARS }; /* |r|^2 alternates between two cells (as in cg_amd.c) */

typedef struct Cg {
    spgpuHandle_t h;
    int n, hackSize, avgNnz;
    double *dV, *dX, *dR, *dP, *dAp, *dS;
    int *dI, *dHo, *dRs;
} Cg;

/* one CG iteration with the scalars on the device; rrOld / rrNew: the two |r|^2 cells */
static void iteration(const Cg* c, double* rrOld, double* rrNew)
{
    spgpuDhellspmv(c->h, c->dAp, c->dAp, 1.0, c->dV, c->dI, c->hackSize, c->dHo, c->dRs, NULL, c->avgNnz, c->n, c->dP, 0.0, 0); /* Ap = A p */
    spgpuDdotDevice(c->h, c->dS + PAP, c->n, c->dP, c->dAp);
    spgpuDaxpbyQuotDevice(c->h, c->dX, c->n, NULL, NULL, c->dX, rrOld, c->dS + PAP, 0, c->dP);   /* x += (rr/pAp) p    */
    spgpuDaxpbyQuotDevice(c->h, c->dR, c->n, NULL, NULL, c->dR, rrOld, c->dS + PAP, 1, c->dAp);  /* r -= (rr/pAp) Ap   */
    spgpuDdotDevice(c->h, rrNew, c->n, c->dR, c->dR);
    spgpuDaxpbyQuotDevice(c->h, c->dP, c->n, rrNew, rrOld, c->dP, NULL, NULL, 0, c->dR);         /* p = r + (rr'/rr) p */
}

/* x = 0, r = p = b, |r|^2 into RR_A */
static void restart(const Cg* c, const double* b)
{
    CHECK(hipMemcpy(c->dR, b, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(c->dP, b, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemset(c->dX, 0, (size_t)c->n * sizeof(double)));
    spgpuDdotDevice(c->h, c->dS + RR_A, c->n, c->dR, c->dR);
    CHECK(hipStreamSynchronize(spgpuGetStream(c->h)));
}

/* k iterations replayed from one captured graph per parity; *uses: spgpuSpmvAdoptedUses gained by the two captures */
static float graphRun(const Cg* c, const double* b, int k, int* uses)
{
    hipStream_t stream = spgpuGetStream(c->h);
    hipGraph_t graph[2];
    hipGraphExec_t step[2];
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    restart(c, b);
    const int before = spgpuSpmvAdoptedUses(c->h);
    for (int parity = 0; parity < 2; ++parity) {
        CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeGlobal));
        iteration(c, c->dS + (parity ? RR_B : RR_A), c->dS + (parity ? RR_A : RR_B));
        CHECK(hipStreamEndCapture(stream, &graph[parity]));
        CHECK(hipGraphInstantiate(&step[parity], graph[parity], NULL, NULL, 0));
    }
    *uses = spgpuSpmvAdoptedUses(c->h) - before;
    CHECK(hipEventRecord(t0, stream));
    for (int i = 0; i < k; ++i)
        CHECK(hipGraphLaunch(step[i & 1], stream));
    CHECK(hipEventRecord(t1, stream));
    CHECK(hipEventSynchronize(t1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    for (int parity = 0; parity < 2; ++parity) {
        CHECK(hipGraphExecDestroy(step[parity]));
        CHECK(hipGraphDestroy(graph[parity]));
    }
    CHECK(hipEventDestroy(t0));
    CHECK(hipEventDestroy(t1));
    printf("  spgpuSpmvAdoptedUses: %d before the captures, %d after\n", before, before + *uses);
    return ms;
}

/* the iterate and |r|^2 after k iterations; 1 if both equal (x0, rr0) bit for bit */
static int sameAs(const Cg* c, int k, const double* x0, double rr0, double* x)
{
    double rr = 0;
    CHECK(hipMemcpy(x, c->dX, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&rr, c->dS + ((k & 1) ? RR_B : RR_A), sizeof(double), hipMemcpyDeviceToHost));
    return memcmp(x, x0, (size_t)c->n * sizeof(double)) == 0 && memcmp(&rr, &rr0, sizeof(double)) == 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s matrix.mtx [iterations=50]\n", argv[0]);
        return 2;
    }
    const char* path = argv[1];
    const int k = argc > 2 ? atoi(argv[2]) : 50;
    const int hackSize = 32;

    /* Matrix Market -> zero-based COO, symmetric storage unfolded */
    int prop[6];
    if (!spgpuMmProperties(path, prop)) {
        fprintf(stderr, "%s: not a readable Matrix Market file\n", path);
        return 2;
    }
    if (prop[0] != prop[1] || prop[5] != 1 /* MATRIX_TYPE_SYMMETRIC */) {
        fprintf(stderr, "%s: CG needs a square matrix in symmetric storage\n", path);
        return 2;
    }
    const int n = prop[0];
    int stored = prop[2];
    int *fr = (int*)malloc((size_t)stored * sizeof(int)), *fc = (int*)malloc((size_t)stored * sizeof(int));
    double* fv = (double*)malloc((size_t)stored * sizeof(double));
    const int code = spgpuMmReadCoo(path, 'd', fv, fr, fc);
    if (code != 0) {
        fprintf(stderr, "%s: read failed with code %d\n", path, code);
        return 2;
    }
    const int nnz = spgpuMmUnfoldedSizeD(fv, fr, fc, stored);
    int *cr = (int*)malloc((size_t)nnz * sizeof(int)), *cc = (int*)malloc((size_t)nnz * sizeof(int));
    double* cv = (double*)malloc((size_t)nnz * sizeof(double));
    spgpuMmUnfoldD(cr, cc, cv, fr, fc, fv, stored);

    /* COO -> ELL -> HELL, rows as they come */
    int maxRow = 0, height = 0;
    int* rowLen = (int*)malloc((size_t)n * sizeof(int));
    computeEllRowLenghts(rowLen, &maxRow, n, nnz, cr, 0);
    const int pitch = computeEllAllocPitch(n);
    double* ev = (double*)calloc((size_t)maxRow * pitch, sizeof(double));
    int* ei = (int*)calloc((size_t)maxRow * pitch, sizeof(int));
    cooToEll(ev, ei, pitch, pitch, maxRow, 0, n, nnz, cr, cc, cv, 0, SPGPU_TYPE_DOUBLE);
    computeHellAllocSize(&height, hackSize, n, rowLen);
    const int hacks = (n + hackSize - 1) / hackSize;
    double* hv = (double*)calloc((size_t)hackSize * height, sizeof(double));
    int* hi = (int*)calloc((size_t)hackSize * height, sizeof(int));
    int* ho = (int*)calloc(hacks, sizeof(int));
    ellToHell(hv, hi, ho, hackSize, ev, ei, pitch, pitch, rowLen, n, SPGPU_TYPE_DOUBLE);
    free(ev);
    free(ei);

    Cg c;
    memset(&c, 0, sizeof(c));
    c.n = n;
    c.hackSize = hackSize;
    c.avgNnz = (nnz + n - 1) / n;
    CHECK(hipMalloc((void**)&c.dV, (size_t)hackSize * height * sizeof(double)));
    CHECK(hipMalloc((void**)&c.dI, (size_t)hackSize * height * sizeof(int)));
    CHECK(hipMalloc((void**)&c.dHo, hacks * sizeof(int)));
    CHECK(hipMalloc((void**)&c.dRs, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&c.dX, (size_t)n * sizeof(double)));
    CHECK(hipMalloc((void**)&c.dR, (size_t)n * sizeof(double)));
    CHECK(hipMalloc((void**)&c.dP, (size_t)n * sizeof(double)));
    CHECK(hipMalloc((void**)&c.dAp, (size_t)n * sizeof(double)));
    CHECK(hipMalloc((void**)&c.dS, SCALARS * sizeof(double)));
    CHECK(hipMemcpy(c.dV, hv, (size_t)hackSize * height * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(c.dI, hi, (size_t)hackSize * height * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(c.dHo, ho, hacks * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(c.dRs, rowLen, (size_t)n * sizeof(int), hipMemcpyHostToDevice));

    /* b = A * ones: the exact solution is ones */
    double* b = (double*)calloc(n, sizeof(double));
    for (int e = 0; e < nnz; ++e)
        b[cr[e]] += cv[e];

    if (spgpuCreate(&c.h, 0) != SPGPU_SUCCESS)
        return 2;
    printf("CG on %s: %d rows, %d nnz (longest row %d), HELL hackSize %d, rows as they come\n", path, n, nnz, maxRow, hackSize);
    if (spgpuHellSpmvAdopt(c.h, SPGPU_TYPE_DOUBLE, c.dV, c.dI, hackSize, c.dHo, c.dRs, n, 0) != SPGPU_SUCCESS) {
        printf("spgpuHellSpmvAdopt refused the matrix (rows not ragged enough?)\nFAILED\n");
        spgpuDestroy(c.h);
        return 1;
    }
    printf("adopted: the library's ordered copy holds %lld bytes\n", spgpuSpmvFrozenBytes(c.h));
    hipStream_t stream = spgpuGetStream(c.h);
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));

    /* 1. eager, scalars on the device */
    restart(&c, b);
    double rr0 = 0;
    CHECK(hipMemcpy(&rr0, c.dS + RR_A, sizeof(double), hipMemcpyDeviceToHost));
    const int usesEager = spgpuSpmvAdoptedUses(c.h);
    CHECK(hipEventRecord(t0, stream));
    for (int i = 0; i < k; ++i)
        iteration(&c, c.dS + ((i & 1) ? RR_B : RR_A), c.dS + ((i & 1) ? RR_A : RR_B));
    CHECK(hipEventRecord(t1, stream));
    CHECK(hipEventSynchronize(t1));
    float msEager = 0;
    CHECK(hipEventElapsedTime(&msEager, t0, t1));
    double* x0 = (double*)malloc((size_t)n * sizeof(double));
    double* x = (double*)malloc((size_t)n * sizeof(double));
    double rrEager = 0;
    CHECK(hipMemcpy(x0, c.dX, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&rrEager, c.dS + ((k & 1) ? RR_B : RR_A), sizeof(double), hipMemcpyDeviceToHost));
    double err = 0;
    for (int i = 0; i < n; ++i)
        err = fabs(x0[i] - 1.0) > err ? fabs(x0[i] - 1.0) : err;
    printf("eager (device scalars): %d iterations, %.1f us per iteration, %d SpMVs on the adopted copy, relative residual %.3e, max |x - 1| = %.3e\n",
           k, k ? msEager * 1e3 / k : 0.0, spgpuSpmvAdoptedUses(c.h) - usesEager, sqrt(rrEager / rr0), err);

    /* 2. captured, no hold */
    printf("graph, no hold:\n");
    int usesPlain = 0;
    const float msPlain = graphRun(&c, b, k, &usesPlain);
    const int samePlain = sameAs(&c, k, x0, rrEager, x);
    printf("graph, no hold: %.1f us per iteration; x and |r|^2 %s\n", k ? msPlain * 1e3 / k : 0.0,
           samePlain ? "bit-identical to the eager run" : "differ from the eager run (the plain kernel: another order of additions)");

    /* 3. captured under a hold */
    const int held = spgpuSpmvHold(c.h, c.dI);
    printf("graph, held (spgpuSpmvHold: %d, holds %d):\n", held, spgpuSpmvHolds(c.h, c.dI));
    int usesHeld = 0;
    const float msHeld = graphRun(&c, b, k, &usesHeld);
    const int sameHeld = sameAs(&c, k, x0, rrEager, x);
    printf("graph, held: %.1f us per iteration; x and |r|^2 %s\n", k ? msHeld * 1e3 / k : 0.0,
           sameHeld ? "bit-identical to the eager run" : "DIFFER from the eager run");
    const int thawHeld = spgpuSpmvThaw(c.h, c.dI); /* the graphs are gone, but the hold is not: refused */
    const int released = spgpuSpmvRelease(c.h, c.dI);
    const int thawed = spgpuSpmvThaw(c.h, c.dI);
    printf("Thaw under the hold: %d (SPGPU_IN_USE = %d); Release: %d; Thaw: %d\n", thawHeld, SPGPU_IN_USE, released, thawed);

    spgpuDestroy(c.h);
    CHECK(hipGetLastError());
    const int ok = rrEager < rr0 && held == SPGPU_SUCCESS && sameHeld && usesHeld == 2 && usesPlain == 0 && thawHeld == SPGPU_IN_USE &&
                   released == SPGPU_SUCCESS && thawed == SPGPU_SUCCESS;
    printf(ok ? "PASSED\n" : "FAILED (residual did not fall, the held graph differs from the eager run, or a count is off)\n");
    return ok ? 0 : 1;
}
