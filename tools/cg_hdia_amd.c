/*
 * Conjugate gradient on a matrix kept in HDIA, written against the C ABI only: the captured iteration with the fused
 * spgpuDhdiaspmvDotDevice (spgpu/ext/hdia_solver.h) against the same iteration from spgpuDhdiaspmv + spgpuDdotDevice.
 * A = the 7-point Laplacian on a g x g x g grid, COO -> HDIA on the host (computeHdiaHackOffsetsFromCoo, cooToHdia), hackSize 32.
 * x0 = 0, b = A * ones.  `iters` fixed iterations, each one launch of a captured graph (two graphs that alternate: the scalar
 * cells of an iteration are the other one's old cells), in two legs:
 *   unfused  spgpuDhdiaspmv, spgpuDdotDevice, 2 x spgpuDaxpbyQuotDevice, spgpuDdotDevice, spgpuDaxpbyQuotDevice: 8 kernels;
 *   fused    spgpuDhdiaspmvDotDevice, spgpuDaxpbyPairDotDevice, spgpuDaxpbyQuotDevice: 5 kernels.
 * With `jacobi` the matrix is A = S L S, S = diag(s_i), s_i = 10^(3 u_i - 1.5) (tools/pcg_amd.c), and both legs run Jacobi-PCG:
 * dinv from spgpuDhdiaDiag(..., invert = 1), the start from spgpuDaxyDotDevice, the update spgpuDaxpbyPairAxyDotDevice and
 * spgpuDaxpbyQuotDevice (spgpu/ext/precond.h); the legs differ in the SpMV and its dot only (6 kernels against 5).
 * The iterate x and the last |r|^2 of the two legs must be identical bit for bit, and |r|^2 must have fallen below its start.
 *
 *   usage: cg_hdia_amd [g=64] [iters=30] [jacobi]
 * Prints the time per iteration of each leg and PASSED / FAILED; exits 0 iff PASSED.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/hdia.h"
#include "spgpu/hdia_conv.h"
#include "spgpu/vector.h"
#include "spgpu/device_scalars.h"
#include "spgpu/ext/hdia_solver.h"
#include "spgpu/ext/precond.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

/* a small linear congruential generator (Numerical Recipes' constants): u in [0, 1) from the upper 24 bits */
static unsigned lcgState = 12345u;
static double lcgUniform(void)
{
    lcgState = lcgState * 1664525u + 1013904223u;
    return (double)(lcgState >> 8) / 16777216.0;
}

enum { RZ_A, RR_A, RZ_B, RR_B, PAP, SCALARS }; /* (r.z, |r|^2) alternates between two pairs of cells; plain CG keeps |r|^2 in the first of a pair */

typedef struct {
    spgpuHandle_t h;
    int n, hackSize, jacobi;
    double *dM, *x, *r, *p, *Ap, *z, *dinv, *cells;
    int *offsets, *hackOffsets;
    const double* b;
} Solver;

/* one iteration on the handle's stream; cells of parity 0: old = A, new = B */
static void iteration(const Solver* s, int parity, int fused)
{
    double* old = s->cells + (parity ? RZ_B : RZ_A);
    double* now = s->cells + (parity ? RZ_A : RZ_B);
    double* pAp = s->cells + PAP;
    if (fused) {
        spgpuDhdiaspmvDotDevice(s->h, pAp, NULL, s->Ap, NULL, 1.0, s->dM, s->offsets, s->hackSize, s->hackOffsets, s->n, s->n, s->p, 0.0);
    } else {
        spgpuDhdiaspmv(s->h, s->Ap, NULL, 1.0, s->dM, s->offsets, s->hackSize, s->hackOffsets, s->n, s->n, s->p, 0.0);
        spgpuDdotDevice(s->h, pAp, s->n, s->p, s->Ap);
    }
    if (s->jacobi) {
        spgpuDaxpbyPairAxyDotDevice(s->h, now, s->n, s->x, s->x, s->p, s->r, s->r, s->Ap, s->z, s->dinv, old, pAp);
        spgpuDaxpbyQuotDevice(s->h, s->p, s->n, now, old, s->p, NULL, NULL, 0, s->z);      /* p = z + (r.z / r.z old) p */
        return;
    }
    if (fused) {
        spgpuDaxpbyPairDotDevice(s->h, now, s->n, s->x, s->x, s->p, s->r, s->r, s->Ap, old, pAp);
    } else {
        spgpuDaxpbyQuotDevice(s->h, s->x, s->n, NULL, NULL, s->x, old, pAp, 0, s->p);      /* x += (|r|^2 / p.Ap) p */
        spgpuDaxpbyQuotDevice(s->h, s->r, s->n, NULL, NULL, s->r, old, pAp, 1, s->Ap);     /* r -= (|r|^2 / p.Ap) Ap */
        spgpuDdotDevice(s->h, now, s->n, s->r, s->r);
    }
    spgpuDaxpbyQuotDevice(s->h, s->p, s->n, now, old, s->p, NULL, NULL, 0, s->r);          /* p = r + (|r|^2 / |r|^2 old) p */
}

/* `iters` iterations from x = 0; returns the microseconds per iteration, x in xOut, the last |r|^2 in *rrOut */
static double leg(const Solver* s, int fused, int iters, double* xOut, double* rrOut)
{
    const size_t vecBytes = (size_t)s->n * sizeof(double);
    hipStream_t stream = spgpuGetStream(s->h);
    CHECK(hipMemcpy(s->r, s->b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(s->x, 0, vecBytes));
    CHECK(hipMemset(s->cells, 0, SCALARS * sizeof(double)));
    if (s->jacobi) {
        spgpuDaxyDotDevice(s->h, s->cells + RZ_A, s->n, s->z, s->dinv, s->r);              /* z = M^-1 r, r.z */
        CHECK(hipMemcpyAsync(s->p, s->z, vecBytes, hipMemcpyDeviceToDevice, stream));
    } else {
        spgpuDdotDevice(s->h, s->cells + RZ_A, s->n, s->r, s->r);
        CHECK(hipMemcpyAsync(s->p, s->r, vecBytes, hipMemcpyDeviceToDevice, stream));
    }
    hipGraph_t graph[2];
    hipGraphExec_t step[2];
    for (int parity = 0; parity < 2; ++parity) {
        CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeGlobal));
        iteration(s, parity, fused);
        CHECK(hipStreamEndCapture(stream, &graph[parity]));
        CHECK(hipGraphInstantiate(&step[parity], graph[parity], NULL, NULL, 0));
    }
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    CHECK(hipEventRecord(t0, stream));
    for (int i = 0; i < iters; ++i)
        CHECK(hipGraphLaunch(step[i & 1], stream));
    CHECK(hipEventRecord(t1, stream));
    CHECK(hipEventSynchronize(t1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    double last[2] = {0, 0};
    CHECK(hipMemcpy(xOut, s->x, vecBytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(last, s->cells + ((iters & 1) ? RZ_B : RZ_A), sizeof(last), hipMemcpyDeviceToHost));
    *rrOut = last[s->jacobi ? 1 : 0];
    for (int parity = 0; parity < 2; ++parity) {
        CHECK(hipGraphExecDestroy(step[parity]));
        CHECK(hipGraphDestroy(graph[parity]));
    }
    CHECK(hipEventDestroy(t0));
    CHECK(hipEventDestroy(t1));
    return ms * 1e3 / iters;
}

int main(int argc, char** argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 64;
    const int iters = argc > 2 ? atoi(argv[2]) : 30;
    const int jacobi = argc > 3 && strcmp(argv[3], "jacobi") == 0;
    if (g < 2 || g > 512 || iters < 1 || (argc > 3 && !jacobi)) {
        fprintf(stderr, "usage: cg_hdia_amd [g=64] [iters=30] [jacobi]\n");
        return 2;
    }
    const int n = g * g * g, hackSize = 32;

    double* scale = (double*)malloc((size_t)n * sizeof(double));
    for (int i = 0; i < n; ++i)
        scale[i] = jacobi ? pow(10.0, 3.0 * lcgUniform() - 1.5) : 1.0;

    /* A = S L S in COO, natural order: entry (i, j) = (s_i * L_ij) * s_j */
    int nnz = 0;
    int* cr = (int*)malloc((size_t)7 * n * sizeof(int));
    int* cc = (int*)malloc((size_t)7 * n * sizeof(int));
    double* cv = (double*)malloc((size_t)7 * n * sizeof(double));
#define ENTRY(j, l) { cr[nnz] = i; cc[nnz] = (j); cv[nnz++] = (scale[i] * (l)) * scale[j]; }
    for (int i = 0; i < n; ++i) {
        const int gx = i % g, gy = i / g % g, gz = i / (g * g);
        if (gz > 0)     ENTRY(i - g * g, -1.0)
        if (gy > 0)     ENTRY(i - g, -1.0)
        if (gx > 0)     ENTRY(i - 1, -1.0)
        ENTRY(i, 6.0)
        if (gx < g - 1) ENTRY(i + 1, -1.0)
        if (gy < g - 1) ENTRY(i + g, -1.0)
        if (gz < g - 1) ENTRY(i + g * g, -1.0)
    }
#undef ENTRY
    const int hacks = getHdiaHacksCount(hackSize, n);
    int height = 0;
    int* ho = (int*)calloc((size_t)hacks + 1, sizeof(int));
    computeHdiaHackOffsetsFromCoo(&height, ho, hackSize, n, n, nnz, cr, cc, 0);
    double* hv = (double*)calloc((size_t)hackSize * height, sizeof(double));
    int* hoff = (int*)calloc((size_t)height, sizeof(int));
    cooToHdia(hv, hoff, ho, hackSize, n, n, nnz, cr, cc, cv, 0, SPGPU_TYPE_DOUBLE);

    /* b = A * ones: the exact solution is ones */
    double* b = (double*)calloc(n, sizeof(double));
    double rr0 = 0;
    for (int e = 0; e < nnz; ++e)
        b[cr[e]] += cv[e];
    for (int i = 0; i < n; ++i)
        rr0 += b[i] * b[i];

    const size_t vecBytes = (size_t)n * sizeof(double);
    Solver s;
    s.n = n;
    s.hackSize = hackSize;
    s.jacobi = jacobi;
    s.b = b;
    if (spgpuCreate(&s.h, 0) != SPGPU_SUCCESS) return 2;
    CHECK(hipMalloc((void**)&s.dM, (size_t)hackSize * height * sizeof(double)));
    CHECK(hipMalloc((void**)&s.offsets, (size_t)height * sizeof(int)));
    CHECK(hipMalloc((void**)&s.hackOffsets, ((size_t)hacks + 1) * sizeof(int)));
    CHECK(hipMalloc((void**)&s.x, vecBytes));
    CHECK(hipMalloc((void**)&s.r, vecBytes));
    CHECK(hipMalloc((void**)&s.p, vecBytes));
    CHECK(hipMalloc((void**)&s.Ap, vecBytes));
    CHECK(hipMalloc((void**)&s.z, vecBytes));
    CHECK(hipMalloc((void**)&s.dinv, vecBytes));
    CHECK(hipMalloc((void**)&s.cells, SCALARS * sizeof(double)));
    CHECK(hipMemcpy(s.dM, hv, (size_t)hackSize * height * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(s.offsets, hoff, (size_t)height * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(s.hackOffsets, ho, ((size_t)hacks + 1) * sizeof(int), hipMemcpyHostToDevice));
    printf("%s on %s, L the %d^3 7-point Laplacian (%d rows, %d nnz), HDIA hackSize %d, %d stored diagonals, %d iterations\n",
           jacobi ? "Jacobi-PCG" : "CG", jacobi ? "A = S L S" : "A = L", g, n, nnz, hackSize, height, iters);

    int dinvWrong = 0;
    if (jacobi) {
        spgpuDhdiaDiag(s.h, s.dinv, s.dM, s.offsets, hackSize, s.hackOffsets, n, n, 1);
        double* dinv = (double*)malloc(vecBytes);
        CHECK(hipMemcpy(dinv, s.dinv, vecBytes, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            const double want = 1.0 / ((scale[i] * 6.0) * scale[i]);
            dinvWrong += memcmp(&want, &dinv[i], sizeof(double)) != 0;
        }
        printf("dinv from spgpuDhdiaDiag: %s the host's 1 / (6 s_i^2) (%d of %d differ)\n", dinvWrong ? "DIFFERS from" : "equal to",
               dinvWrong, n);
        free(dinv);
    }

    double* xUnfused = (double*)malloc(vecBytes);
    double* xFused = (double*)malloc(vecBytes);
    double rrUnfused = 0, rrFused = 0;
    leg(&s, 0, iters, xUnfused, &rrUnfused); /* warm-up: code objects loaded, caches filled */
    const double usUnfused = leg(&s, 0, iters, xUnfused, &rrUnfused);
    leg(&s, 1, iters, xFused, &rrFused);
    const double usFused = leg(&s, 1, iters, xFused, &rrFused);
    double err = 0;
    for (int i = 0; i < n; ++i)
        if (fabs(xFused[i] - 1.0) > err)
            err = fabs(xFused[i] - 1.0);
    const int sameX = memcmp(xUnfused, xFused, vecBytes) == 0;
    const int sameRr = memcmp(&rrUnfused, &rrFused, sizeof(double)) == 0;
    const int fallen = rrFused < rr0 && rrUnfused < rr0; /* false for a NaN too */
    printf("unfused: %.1f us per iteration (%d kernels), |r|^2 %.6e -> %.6e\n", usUnfused, jacobi ? 6 : 8, rr0, rrUnfused);
    printf("fused:   %.1f us per iteration (5 kernels), |r|^2 %.6e -> %.6e, max |x - 1| = %.3e\n", usFused, rr0, rrFused, err);
    printf("x %s, |r|^2 %s, |r|^2 %s\n", sameX ? "same" : "DIFFERS", sameRr ? "same" : "DIFFERS", fallen ? "has fallen" : "has NOT fallen");

    spgpuDestroy(s.h);
    CHECK(hipGetLastError());
    const int ok = sameX && sameRr && fallen && dinvWrong == 0;
    printf(ok ? "PASSED\n" : "FAILED (the fused leg differs from the unfused one, |r|^2 did not fall, or dinv is not the host's)\n");
    return ok ? 0 : 1;
}
